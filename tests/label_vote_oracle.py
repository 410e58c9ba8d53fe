"""NumPy restatement of the Cityscapes output stage behind a label-image segmentation — the reference's --lrr_seg path — written
from postprocess.py:5-52, 109-145, cityscapes_eval.py:162-164, 183-189, 212-232 and analysis.py:232-261; no device.  The test
helper of test_label_vote*.py.

The label image becomes a one-hot map [H,W,9] (:228-231: channel 1 + i = "label == sem_ids[i]", channel 0 = 1 - max), the
foreground mask is 1 - channel 0 (:164), and the vote (seg[..., None] * fg_h).mean(0).mean(0) of a binary mask counts, per
class, its pixels — so everything here is integer counting, and the integers define the class.

One case is the library's rule and not the reference's: below zero the reference's `one_label > thresh` (postprocess.py:12 on
the output of :48) is also true on every plane that LOST the arg-max, whose one-label value is 0; here, as in the kernels, only
the arg-max plane of a pixel is ever marked.  The default threshold list has no negative entry."""
import numpy as np

LABEL_IDS = (24, 25, 26, 27, 28, 31, 32, 33)  # analysis.py:203-210
CLASS_IDS = {'labelIds': LABEL_IDS, 'trainIds': tuple(range(11, 19)), 'lrr': (12, 13, 14, 15, 16, 17, 18, 19)}  # :213-216


def class_lut(ids):
  lut = np.zeros(256, np.uint8)
  for c, v in enumerate(CLASS_IDS[ids]):
    lut[v] = c + 1
  return lut


def onehot(labels, lut):
  """:228-231 for labels uint8 [B,H,W] -> float64 [B,H,W,9]."""
  cls = np.asarray(lut)[np.asarray(labels)]
  fg = np.zeros(cls.shape + (9,), np.float64)
  for ii in range(8):
    fg[..., ii + 1] = cls == ii + 1
  fg[..., 0] = 1 - fg.max(axis=-1)
  return fg


def one_label(y):
  """postprocess.py:45: (t* [B,H,W], v = y[b,t*,p]); the first maximum."""
  y = np.asarray(y, np.float32)
  am = np.argmax(y, axis=1)
  return am, np.take_along_axis(y, am[:, None], axis=1)[:, 0]


def planes(y, labels, lut, thresh, keep=None):
  """One threshold's binary planes [B,T,H,W] float32: one label -> threshold (strict, float32) -> foreground -> keep [B,T]."""
  y = np.asarray(y, np.float32)
  am, v = one_label(y)
  on = (v > np.float32(thresh)) & (np.asarray(lut)[np.asarray(labels)] > 0)
  out = (np.arange(y.shape[1])[None, :, None, None] == am[:, None]) & on[:, None]
  if keep is not None:
    out = out & (np.asarray(keep) != 0)[:, :, None, None]
  return out.astype(np.float32)


def sweep(y_f32, labels, lut, thresholds, conf, remove_tiny):
  """Everything the sweep and its finishing launch return, with a leading K axis, walking the thresholds in list order:
  counts int64 [K,B,T,8], sizes int64 [K,B,T], keep uint8, conf float32, vote float32 [K,B,T,9], class_idx, label_id int32."""
  y = np.asarray(y_f32, np.float32)
  B, T, H, W = y.shape
  K = len(thresholds)
  cls = np.asarray(lut)[np.asarray(labels)].astype(np.int64)       # [B,H,W], 0 = background
  am, v = one_label(y)
  counts = np.zeros((K, B, T, 8), np.int64)
  for k, th in enumerate(thresholds):
    on = (v > np.float32(th)) & (cls > 0)                           # postprocess.py:12 (float32), :145 with fg of :164
    for b in range(B):
      flat = am[b][on[b]] * 8 + cls[b][on[b]] - 1
      counts[k, b] = np.bincount(flat, minlength=T * 8).reshape(T, 8)
  sizes = counts.sum(-1)
  keep = np.zeros((K, B, T), np.uint8)
  cf = np.zeros((K, B, T), np.float32)
  vote = np.zeros((K, B, T, 9), np.float32)
  idx = -np.ones((K, B, T), np.int32)
  lab = -np.ones((K, B, T), np.int32)
  c = np.asarray(conf, np.float32).copy()
  for k in range(K):
    keep[k] = 1 if remove_tiny == 0 else sizes[k] > remove_tiny     # postprocess.py:115,131
    c = c * keep[k].astype(np.float32)                              # :132, and cityscapes_eval.py:188-189 carries it on
    cf[k] = c
    vote[k, ..., 1:] = (counts[k].astype(np.float64) / float(H * W)).astype(np.float32) * keep[k][..., None]
    written = c > 0.5                                               # analysis.py:236; :252 is always open (vote[0] = 0)
    first = np.argmax(counts[k], axis=-1)                           # :253 on the counts
    idx[k] = np.where(written, first, -1)
    lab[k] = np.where(written, np.asarray(LABEL_IDS)[first], -1)
  return {'counts': counts, 'sizes': sizes, 'keep': keep, 'conf': cf, 'vote': vote, 'class_idx': idx, 'label_id': lab}


def text_lines(name, conf, label_id, class_idx):
  """analysis.py:254-259 for one image: [(png name, label id, score)] of the written instances."""
  stem = name[:-4] if name.endswith('.png') else name
  return [('%s_%03d.png' % (stem, t), int(label_id[t]), float(conf[t])) for t in range(len(class_idx)) if class_idx[t] >= 0]


# ---- inputs the tests share ----
def scene(seed, B, T, H, W, thresholds, grid=64):
  """Masks on a grid of multiples of 1 / grid in [0, 1] (so no value sits on a threshold unless put there), with exact zeros,
  ties over T and all-zero pixels; then, per threshold, some pixels exactly at float32(th) and some one ulp above; a label
  image of thing labels, stuff labels and 255."""
  rng = np.random.RandomState(seed)
  y = (rng.randint(0, grid + 1, (B, T, H, W)) / float(grid)).astype(np.float32)
  y[rng.rand(B, T, H, W) < 0.3] = 0.0
  dead = rng.rand(B, H, W) < 0.15
  y[np.broadcast_to(dead[:, None], y.shape)] = 0.0                  # all-zero pixels: arg-max 0
  if T > 1:
    tie = rng.rand(B, H, W) < 0.15
    top = y.max(axis=1)
    y[:, T - 1][tie] = top[tie]                                     # the last instance ties the maximum: the first one wins
  flat = y.reshape(B, T, H * W)
  for k, th in enumerate(thresholds):
    f = np.float32(th)
    for j, val in enumerate((f, np.nextafter(f, np.float32(np.inf), dtype=np.float32))):
      p = rng.randint(0, H * W, 3)
      flat[:, :, p] = np.minimum(flat[:, :, p], val)                # nothing above it there ...
      flat[rng.randint(0, B), rng.randint(0, T), p] = val           # ... and one instance exactly on it
  pool = np.array(list(LABEL_IDS) + [0, 7, 11, 23, 29, 30, 255], np.uint8)
  blocks = pool[rng.randint(0, len(pool), (B, (H + 3) // 4, (W + 7) // 8))]
  labels = np.repeat(np.repeat(blocks, 4, axis=1), 8, axis=2)[:, :H, :W]
  noise = rng.rand(B, H, W) < 0.1
  labels = np.where(noise, pool[rng.randint(0, len(pool), (B, H, W))], labels).astype(np.uint8)
  conf = rng.uniform(0.3, 1.0, (B, T)).astype(np.float32)
  return np.ascontiguousarray(y), np.ascontiguousarray(labels), conf
