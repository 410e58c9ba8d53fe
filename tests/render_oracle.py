"""NumPy restatement of the reference's render analyzers (analysis.py:67-193, 270-283; data_api/orientation.py:3-28;
fg_model_eval.py:128-132), written from those lines; the test helper of test_render*.py.  The reference computes in uint8
arrays, whose products and sums wrap; here that wrap-around is spelled out with `& 255` on int64, so nothing depends on
NumPy's overflow behaviour.  Images are returned as cv2.imwrite receives them: [.., H, W, 3] in B, G, R memory order, which
is what utils/png.read_colour8 gives back for the written file."""
import numpy as np

import cs_oracle as cso
import pixel_oracle as po

# analysis.py:103-124; the last row's 319 is stored in a uint8 array there: 319 & 255 = 63
CMAP = np.array([[192, 57, 43], [243, 156, 18], [26, 188, 156], [41, 128, 185], [142, 68, 173], [44, 62, 80], [127, 140, 141],
                 [17, 75, 95], [2, 128, 144], [228, 253, 225], [69, 105, 144], [244, 91, 105], [91, 192, 235], [253, 231, 76],
                 [155, 197, 61], [229, 89, 52], [250, 121, 33], [124, 82, 47], [86, 15, 94], [38, 63, 77], [1, 52, 55],
                 [319 & 255, 29, 82]], np.int64)
# data_api/orientation.py:3-11
WHEEL = np.array([[255, 17, 0], [255, 137, 0], [230, 255, 0], [34, 255, 0], [0, 255, 213], [0, 154, 255], [9, 0, 255],
                  [255, 0, 255]], np.int64)


def as_u8(v):
  """.astype('uint8') of a finite 0 <= v <= 255: truncation, then mod 256."""
  return np.trunc(np.asarray(v, np.float64)).astype(np.int64) & 255


def add_image(y, colours):
  """analysis.py:137-147 for one image BEFORE the channel swap: y [T,H,W], colours [T,3] (the colour of plane t) -> int64
  [H,W,3] of bytes.  `size > 0` gates nothing: an empty plane adds zero."""
  total = np.zeros(y.shape[1:] + (3,), np.int64)
  for t in range(y.shape[0]):
    prod = (as_u8(y[t])[:, :, None] * np.asarray(colours[t], np.int64)) & 255  # the uint8 product wraps
    total = (total + prod) & 255                                               # and so does the uint8 +=
  return total


def first_image(y, colours):
  """analysis.py:166-185 for one image BEFORE the channel swap: total += (total == 0) * y_t * colour, all uint8, so the
  `== 0` is decided per CHANNEL."""
  total = np.zeros(y.shape[1:] + (3,), np.int64)
  for t in range(y.shape[0]):
    prod = ((total == 0).astype(np.int64) * as_u8(y[t])[:, :, None]) & 255
    prod = (prod * np.asarray(colours[t], np.int64)) & 255
    total = (total + prod) & 255
  return total


def render_instances(y, colours=None):
  """RenderInstanceAnalyzer.stage for a batch y [B,T,H,W] -> uint8 [B,H,W,3] as handed to cv2.imwrite (:147: swapped, so the
  file's R, G, B is the cmap row).  colours: [T,3] or [B,T,3] rows in the CMAP's order; None = CMAP[t % 22] (:144)."""
  y = np.asarray(y)
  B, T = y.shape[:2]
  if colours is None:
    colours = CMAP[np.arange(T) % CMAP.shape[0]]
  colours = np.broadcast_to(np.asarray(colours, np.int64), (B, T, 3))
  return np.stack([add_image(y[b], colours[b])[:, :, [2, 1, 0]] for b in range(B)]).astype(np.uint8)


def groundtruth_colours(iou_pairwise):
  """analysis.py:164-182 for a batch: iou_pairwise [B,T_out,T_gt] -> int64 [B,T_gt,3] CMAP rows.  flag[max_idx] raises
  IndexError for max_idx >= 22, as the reference's does."""
  iou = np.asarray(iou_pairwise)
  n = CMAP.shape[0]
  out = np.zeros((iou.shape[0], iou.shape[2], 3), np.int64)
  for ii in range(iou.shape[0]):
    flag = np.zeros(n)
    color = None
    for jj in range(iou.shape[2]):
      max_idx = np.argmax(iou[ii][:, jj])
      if flag[max_idx] == 0:
        color = CMAP[max_idx]
        flag[max_idx] = 1
      else:
        for kk in range(n):
          idx = n - kk - 1
          if flag[idx] == 0:
            color = CMAP[idx]
            flag[idx] = 1
            break
      out[ii, jj] = color
  return out


def render_groundtruth(y_gt, iou_pairwise):
  """RenderGroundtruthInstanceAnalyzer.stage for a batch -> uint8 [B,H,W,3] as handed to cv2.imwrite (:187: swapped)."""
  y_gt = np.asarray(y_gt)
  colours = groundtruth_colours(iou_pairwise)
  return np.stack([first_image(y_gt[b], colours[b])[:, :, [2, 1, 0]] for b in range(y_gt.shape[0])]).astype(np.uint8)


def orientation_full(d, H, W):
  """fg_model_eval.py:128-132 in float64: d [B,Hs,Ws,C] -> [B,H,W,C], every channel through cv2.resize(.., (W, H))."""
  return cso.sem_full(d, H, W)


def orientation_image(d_full, mask):
  """data_api/orientation.py:13-28 on full-size planes d_full [B,H,W,C], mask [B,H,W] of 0 / 1 -> uint8 [B,H,W,3] as handed to
  cv2.imwrite (analysis.py:278-282: NOT swapped, so the file's B, G, R is the wheel row)."""
  did = np.argmax(d_full, axis=-1)
  c2 = WHEEL[did]
  return as_u8(c2 * np.asarray(mask, np.float64)[..., None]).astype(np.uint8)


def orientation_gap(d_full):
  """The difference between the two largest channels: where it is small, float32 and float64 may pick different classes."""
  return po.top2_gap(d_full)


def count_text(indices, y_out, s_gt):
  """CountAnalyzer (:72, :80-86): the file's text for one staged batch."""
  y_out = np.asarray(y_out)
  count_out = (y_out.reshape(y_out.shape[0], y_out.shape[1], -1).sum(axis=2) > 0).astype(np.float32).sum(axis=1)  # f_count_out
  count_gt = np.asarray(s_gt).sum(axis=1)
  return 'Image ID,Count Out,Count GT\n' + ''.join('{},{:d},{:d}\n'.format(idx, int(count_out[ii]), int(count_gt[ii]))
                                                   for ii, idx in enumerate(indices))
