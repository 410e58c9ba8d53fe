"""Float64 NumPy restatement of the Cityscapes output stage (cityscapes_eval.py:148-205 write_log,
analysis.py:196-267 RenderCityScapesOutputAnalyzer), written from those lines; the test helper of
test_cityscapes_stage*.py.  The post-processing steps are ra_oracle's pp_* where they exist."""
import numpy as np

import ra_oracle as ora

FG_THRESHOLD = 0.3  # cityscapes_eval.py:171
LABELS = [('person', 24), ('rider', 25), ('car', 26), ('truck', 27), ('bus', 28), ('train', 31), ('motorcycle', 32),
          ('bicycle', 33)]  # analysis.py:203-210


def taps(n_src, n_dst):
  """cv2.resize INTER_LINEAR along one axis (restated beside ora.pp_upsample's): pixel centres aligned, clamped."""
  f = (np.arange(n_dst) + 0.5) * (n_src / n_dst) - 0.5
  i0 = np.floor(f).astype(int)
  w = f - i0
  lo, hi = i0 < 0, i0 >= n_src - 1
  i0 = np.clip(i0, 0, n_src - 1)
  w = np.where(lo | hi, 0.0, w)
  return i0, np.minimum(i0 + 1, n_src - 1), w


def resize_linear(a, H, W):
  """cv2.resize(plane, (W, H)) on the last two axes of a [..., Hs, Ws]; no bilateral step."""
  a = np.asarray(a, np.float64)
  y0, y1, wy = taps(a.shape[-2], H)
  x0, x1, wx = taps(a.shape[-1], W)
  top = a[..., y0, :][..., :, x0] * (1 - wx) + a[..., y0, :][..., :, x1] * wx
  bot = a[..., y1, :][..., :, x0] * (1 - wx) + a[..., y1, :][..., :, x1] * wx
  return top * (1 - wy)[:, None] + bot * wy[:, None]


def sem_full(sem, H, W):
  """cityscapes_eval.py:166-170: sem [B,Hs,Ws,C] -> [B,H,W,C], every channel resized."""
  return np.moveaxis(resize_linear(np.moveaxis(np.asarray(sem, np.float64), -1, 1), H, W), 1, -1)


def foreground(sem_h, thresh=FG_THRESHOLD):
  """:172-176 on the full-size map [B,H,W,C] -> [B,H,W]."""
  if sem_h.shape[-1] == 1:
    return (sem_h[..., 0] > thresh).astype(np.float64)
  return (sem_h[..., 0] <= 1 - thresh).astype(np.float64)


def vote(y, sem_h):
  """analysis.py:235-237: y [B,T,H,W], sem_h [B,H,W,C] -> [B,T,C], the mean over all H * W pixels."""
  y = np.asarray(y, np.float64)
  B, T, H, W = y.shape
  return np.stack([y[b].reshape(T, H * W) @ sem_h[b].reshape(H * W, -1) for b in range(B)]) / (H * W)


def pick(v, conf):
  """analysis.py:232,251-253: (class_idx [B,T] with -1 = not written, label_id [B,T])."""
  B, T, _ = v.shape
  idx = -np.ones((B, T), int)
  lab = -np.ones((B, T), int)
  for b in range(B):
    for t in range(T):
      if conf[b, t] > 0.5 and v[b, t, 0] <= 0.7:
        idx[b, t] = int(np.argmax(v[b, t, 1:]))
        lab[b, t] = LABELS[idx[b, t]][1] if idx[b, t] < len(LABELS) else -1
  return idx, lab


def top2_gap(v):
  """Difference between the two largest class votes of vote[..., 1:] -> [B,T] (inf with a single class)."""
  s = np.sort(v[..., 1:], axis=-1)
  return s[..., -1] - s[..., -2] if s.shape[-1] > 1 else np.full(s.shape[:-1], np.inf)


def one_label(y_ins, s_out, H, W):
  """:179-181: pp.upsample -> pp.apply_confidence -> pp.apply_one_label (upsample FIRST, as the reference has it)."""
  y = ora.pp_upsample(np.asarray(y_ins, np.float64), H, W)
  y, conf_hard = ora.pp_apply_confidence(y, np.asarray(s_out, np.float64))
  return y, ora.pp_apply_one_label(y), conf_hard


def threshold_chain(one, fg, sem_h, s_out, thresholds, remove_tiny=400):
  """:183-205 + analysis.py:232-261 on the one-label map: per threshold apply_threshold -> mask_foreground -> remove_tiny, with
  conf carried from threshold to threshold (:188-189), then the vote and the pick."""
  conf = np.asarray(s_out, np.float64).copy()
  out = []
  for th in thresholds:
    yb = ora.pp_apply_threshold(one, th).astype(np.float64) * fg[:, None]
    sizes = yb.sum(axis=(2, 3))
    yb, conf = ora.pp_remove_tiny(yb, conf, remove_tiny)
    v = vote(yb, sem_h)
    idx, lab = pick(v, conf)
    out.append({'threshold': th, 'y_out': yb, 'conf': np.array(conf), 'vote': v, 'class_idx': idx, 'label_id': lab, 'sizes': sizes})
  return out


def label_instances(y_ins, s_out, sem, size, thresholds, remove_tiny=400):
  """Steps 1-4.  One dict per threshold: y_out, conf, vote, class_idx, label_id, sizes (before remove_tiny); plus the shared
  one-label map and its pre-arg-max values for the tests' bands."""
  H, W = size
  sem_h = sem_full(sem, H, W)
  fg = foreground(sem_h)
  y_conf, one, conf_hard = one_label(y_ins, s_out, H, W)
  return {'per_threshold': threshold_chain(one, fg, sem_h, s_out, thresholds, remove_tiny), 'one': one, 'y_conf': y_conf,
          'fg': fg, 'sem_h': sem_h, 'conf_hard': conf_hard}


def text_lines(name, y_out, conf, label_id, class_idx):
  """analysis.py:254-259 for one image: [(png name, label id, score)] of the written instances."""
  stem = name[:-4] if name.endswith('.png') else name
  return [('%s_%03d.png' % (stem, t), int(label_id[t]), float(conf[t])) for t in range(y_out.shape[0]) if class_idx[t] >= 0]


# ---- inputs the tests share ----
def smooth_semantic_map(rng, B, Hs, Ws, C, bg_bias=4.0, quantise=True):
  """A background-biased smooth C-class softmax map through the 8-bit round trip: low-resolution noise, upsampled."""
  h0, w0 = max(2, Hs // 8), max(2, Ws // 8)
  lg = resize_linear(rng.randn(B, C, h0, w0) * 3.0, Hs, Ws)
  lg[:, 0] += bg_bias
  e = np.exp(lg - lg.max(axis=1, keepdims=True))
  p = np.moveaxis(e / e.sum(axis=1, keepdims=True), 1, -1)
  if quantise:
    p = (p * 255).astype('uint8').astype('float32') / np.float32(255)
  return np.ascontiguousarray(p, np.float32)


def disc_instances(rng, B, T, H, W, soft=False, rmin=0.06, rmax=0.2):
  """Random discs: soft = overlapping bumps in [0, 1] with exact zeros away from them; else a one-label binary map."""
  yy, xx = np.mgrid[0:H, 0:W]
  y = np.zeros((B, T, H, W), np.float32)
  for b in range(B):
    for t in range(T):
      r = rng.uniform(rmin, rmax) * min(H, W)
      cy, cx = rng.uniform(0, H), rng.uniform(0, W)
      d = np.sqrt((yy - cy) ** 2 + (xx - cx) ** 2)
      y[b, t] = np.clip(1.5 * (1 - d / r), 0, 1)
  if not soft:
    am = y.argmax(axis=1)
    y = ((np.arange(T)[None, :, None, None] == am[:, None]) & (y > 0.3)).astype(np.float32)
  return y


def synthetic_scene(seed, T=8, h=64, w=128, C=9):
  """A seeded scene at network size: T soft discs (values in [0, 1], exact zeros away from them, neighbours overlapping), each
  of a known class; scores with one 0.2 and one exactly 0.5; an 8-bit-quantised semantic map that gives the disc's class
  most of the weight inside a slightly larger, hard-edged disc and the background the rest (with the few levels that
  leaves, no resized background value can land on the foreground threshold 0.7: the tests assert it).
  -> (y_ins [1,T,h,w], s_out [1,T], sem [1,h,w,C], classes [T] as indices into LABELS)."""
  rng = np.random.RandomState(seed)
  yy, xx = np.mgrid[0:h, 0:w]
  y = np.zeros((1, T, h, w), np.float32)
  fgw = np.zeros((h, w, C), np.float64)
  classes = rng.randint(0, C - 1, T)
  cx = (np.arange(T) + 0.5) * w / T + rng.uniform(-3, 3, T)   # a row of discs, wide enough to overlap their neighbours
  cy = h / 2 + rng.uniform(-h / 5, h / 5, T)
  rad = rng.uniform(0.6, 1.0, T) * w / T
  rad[T - 1] = 3.0                                           # a tiny one, for remove_tiny
  for t in range(T):
    d = np.sqrt((yy - cy[t]) ** 2 + (xx - cx[t]) ** 2)
    y[0, t] = np.clip(1.6 * (1 - d / rad[t]), 0, 1) * rng.uniform(0.8, 1.0)
    fgw[..., 1 + classes[t]] = np.maximum(fgw[..., 1 + classes[t]], 0.9 * (d < 1.25 * rad[t]))
  tot = fgw.sum(-1, keepdims=True)
  fgw = fgw / np.maximum(tot / 0.95, 1.0)                     # overlapping classes share at most 0.95
  fgw[..., 0] = 1.0 - fgw[..., 1:].sum(-1)
  sem = (fgw * 255).astype('uint8').astype('float32') / np.float32(255)
  s = rng.uniform(0.7, 1.0, (1, T)).astype(np.float32)
  s[0, 1], s[0, 2] = 0.2, 0.5
  return y, s, np.ascontiguousarray(sem[None], np.float32), classes
