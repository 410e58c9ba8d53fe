"""Float64 NumPy restatement of what evaluates the pre-stage fg_model in the reference, written from those lines:
the loss head and the statistics of fg_model.py:196-246 (with modellib.f_iou_all :171-181, f_ce :418-421, f_bce :424-427),
and the threshold sweep of fg_model_eval.py:134-178 (upsample :89-117 on ra_oracle.pp_upsample, apply_threshold :119-126,
the accumulating analyzers analysis.py:834-906).  The test helper of test_fg_eval*.py; the reference itself (TensorFlow 0.12,
cv2) cannot be run here."""
import numpy as np

import ra_oracle as ora

EPS = 1e-5  # modellib.py:420,426 and :180
SUM_NAMES = ('inter_soft', 'sum_soft', 'sum_gt', 'inter_hard', 'sum_hard', 'seg_ce', 'ori_ce', 'ori_correct', 'mask')


def head(logits, nsc, no):
  """fg_model.py:179-194 on float64: (y_out [..., nsc], d_out [..., no] or None)."""
  l = np.asarray(logits, np.float64)
  y = l[..., :nsc]
  y_out = ora.sigmoid(y) if nsc == 1 else ora.softmax(y)
  return y_out, (ora.softmax(l[..., nsc:]) if no else None)


def f_iou_all(a, b):
  inter = (a * b).sum()
  return inter / (a.sum() + b.sum() - inter + EPS)


def f_ce(y_out, y_gt):
  return -y_gt * np.log(y_out + EPS)


def f_bce(y_out, y_gt):
  return -y_gt * np.log(y_out + EPS) - (1 - y_gt) * np.log(1 - y_out + EPS)


def sums(logits, y_gt, d_gt, nsc, no):
  """The sums the statistics are made of, {name: float} over SUM_NAMES.  logits [..., nsc + no], y_gt [..., nsc] (or [...]
  with one class), d_gt [..., no] or None."""
  l = np.asarray(logits, np.float64)
  g = np.asarray(y_gt, np.float64).reshape(l.shape[:-1] + (nsc,))
  y_out, d_out = head(l, nsc, no)
  if nsc > 1:
    mask = g[..., 1:nsc].max(axis=-1, keepdims=True)             # :201-203
    hard = (y_out == y_out.max(axis=-1, keepdims=True)).astype(np.float64)  # :213-214
    ys, yh, gs = y_out[..., 1:nsc], hard[..., 1:nsc], g[..., 1:nsc]  # :215-218
    seg = f_ce(y_out, g).sum()                                   # :225
  else:
    mask = g                                                     # :205
    hard = (y_out > 0.5).astype(np.float64)                      # :209
    ys, yh, gs = y_out, hard, g
    seg = f_bce(y_out, g).sum()                                  # :222
  out = {'inter_soft': (ys * gs).sum(), 'sum_soft': ys.sum(), 'sum_gt': gs.sum(), 'inter_hard': (yh * gs).sum(),
         'sum_hard': yh.sum(), 'seg_ce': seg, 'ori_ce': 0.0, 'ori_correct': 0.0, 'mask': 0.0}
  if no:
    d = np.asarray(d_gt, np.float64)
    out['ori_ce'] = (f_ce(d_out, d) * mask).sum()                # :237-238
    correct = (np.argmax(d_out, axis=-1) == np.argmax(d, axis=-1)).astype(np.float64)  # :242, first maximum
    out['ori_correct'] = (correct * mask[..., 0]).sum()          # :244
    out['mask'] = mask.sum()                                     # :206
  return {k: float(v) for k, v in out.items()}


def statistics_of(s, num_pixel, segm_loss_fn, orientation):
  """The six statistics from the sums (fg_model.py:208-248); num_pixel = B * H * W."""
  with np.errstate(divide='ignore', invalid='ignore'):
    f8 = np.float64
    out = {'iou_soft': s['inter_soft'] / (s['sum_soft'] + s['sum_gt'] - s['inter_soft'] + EPS),
           'iou_hard': s['inter_hard'] / (s['sum_hard'] + s['sum_gt'] - s['inter_hard'] + EPS)}
    out['foreground_loss'] = -out['iou_soft'] if segm_loss_fn == 'iou' else s['seg_ce'] / num_pixel  # :228-233
    out['loss'] = out['foreground_loss']
    if orientation:
      out['orientation_ce'] = float(f8(s['ori_ce']) / f8(s['mask']))       # :239
      out['orientation_acc'] = float(f8(s['ori_correct']) / f8(s['mask']))  # :244-245; 0 / 0 = NaN
      out['loss'] = out['foreground_loss'] + out['orientation_ce']          # :240
  return out


def statistics(logits, y_gt, d_gt, nsc, no, segm_loss_fn='iou'):
  l = np.asarray(logits)
  return statistics_of(sums(l, y_gt, d_gt, nsc, no), float(np.prod(l.shape[:-1])), segm_loss_fn, bool(no))


# ---- the threshold sweep
def _reflect101(i, n):
  """BORDER_REFLECT_101 for any offset: ... 2 1 | 0 1 2 ... n-1 | n-2 n-3 ...; a single row or column reflects onto itself."""
  if n == 1:
    return np.zeros_like(i)
  i = np.abs(i) % (2 * (n - 1))
  return np.where(i >= n, 2 * (n - 1) - i, i)


def upsample(src, H, W):
  """fg_model_eval.py:106-117 on [N,Hs,Ws]: cv2.resize(a, (W, H), INTER_LINEAR) then cv2.bilateralFilter(b, 5, 10, 10).
  This is ra_oracle.pp_upsample (tests/test_fg_eval.py holds the two equal) with the border rule written for every size:
  pp_upsample's reflection indexes past the image when H or W is 1, a size the sweep's cases include."""
  import cs_oracle as cso
  b = cso.resize_linear(np.asarray(src, np.float64), H, W)
  rr, cc = np.arange(H), np.arange(W)
  num, den = np.zeros_like(b), np.zeros_like(b)
  for dy in range(-2, 3):
    for dx in range(-2, 3):
      if dy * dy + dx * dx > 4:
        continue
      v = b[..., _reflect101(rr + dy, H), :][..., :, _reflect101(cc + dx, W)]
      wgt = np.exp(-(dy * dy + dx * dx) / (2 * 10.0 ** 2) - (v - b) ** 2 / (2 * 10.0 ** 2))
      num += wgt * v
      den += wgt
  return num / den


def sweep_counts(v, gt, thresholds, shift=0.0):
  """The analyzers' sums for a = [v > threshold + shift] (:126) and b = gt: (count_a [N,K], sum_ab [N,K], sum_b [N]) as int64."""
  gt = np.asarray(gt).astype(np.int64)
  a = [(v > t + shift) for t in thresholds]
  count_a = np.stack([m.sum(axis=(1, 2)) for m in a], axis=1).astype(np.int64)
  sum_ab = np.stack([(m * gt).sum(axis=(1, 2)) for m in a], axis=1).astype(np.int64)
  return count_a, sum_ab, gt.sum(axis=(1, 2))


def fg_iou_all(a_list, b_list):
  """ForegroundIOUAnalyzer (analysis.py:844-866) over lists of [H,W] maps."""
  inter = union = 0.0
  for a, b in zip(a_list, b_list):
    i = (a * b).sum()
    inter += i
    union += a.sum() + b.sum() - i
  return inter / union


def bg_iou_all(a_list, b_list):
  """BackgroundIOUAnalyzer (analysis.py:881-905)."""
  inter = union = 0.0
  for a, b in zip(a_list, b_list):
    _a, _b = 1 - a, 1 - b
    i = (_a * _b).sum()
    inter += i
    union += _a.sum() + _b.sum() - i
  return inter / union


def smooth_map(rng, N, Hs, Ws):
  """An unquantised smooth sigmoid map [N,Hs,Ws] float32: low-resolution Gaussian noise x 4, resized, through a sigmoid."""
  import cs_oracle as cso
  low = rng.randn(N, max(2, Hs // 8), max(2, Ws // 8)) * 4
  return np.ascontiguousarray(ora.sigmoid(cso.resize_linear(low, Hs, Ws)), dtype=np.float32)


def disc_labels(rng, N, H, W, n_disc=5):
  """uint8 [N,H,W]: random discs summed — 2 and more where they overlap."""
  rr, cc = np.mgrid[0:H, 0:W]
  gt = np.zeros((N, H, W), np.int64)
  for n in range(N):
    for _ in range(n_disc):
      cy, cx, rad = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(0.15, 0.35) * max(2, min(H, W))
      gt[n] += ((rr - cy) ** 2 + (cc - cx) ** 2 <= rad ** 2)
  return gt.astype(np.uint8)
