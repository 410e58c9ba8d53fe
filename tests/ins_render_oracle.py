"""NumPy restatement of the pictures on the evaluator's id path: the winner map of the counting pass (one uint16 word
n << 8 | t* per full-size pixel), the pictures painted from it, the ground truth's picture painted from the id image — and
the reference's own composition from masks (analysis.py:137-147: sum over t of uint8(mask_t) * colour_t), which the first
two must reproduce.  The test helper of test_ins_render*.py; the chain in float64 is ins_eval_oracle's."""
import numpy as np

import ins_eval_oracle as ieo


def threshold_pos(thresholds):
  """pos[k] = how many of the thresholds lie strictly below the k-th one given (inse::Order)."""
  thr = np.asarray(thresholds, np.float64)
  return (thr[None, :] < thr[:, None]).sum(axis=1).astype(np.int32)


def map_of(v, thresholds, fg=None, mutant=None):
  """uint16 [B,Hf,Wf] of v = ins_eval_oracle.values(...) in float64: t* = the FIRST maximum over t, n = the thresholds its value
  exceeds with strict > (0 where fg is 0), word n << 8 | t*, 0 where n == 0.  mutant 'last_max': the last maximum takes the
  pixel."""
  T = v.shape[1]
  tstar = T - 1 - np.argmax(v[:, ::-1], axis=1) if mutant == 'last_max' else np.argmax(v, axis=1)
  m = np.take_along_axis(v, tstar[:, None], axis=1)[:, 0]
  n = np.zeros(m.shape, np.int64)
  for th in thresholds:
    n += m > th
  if fg is not None:
    n = n * (np.asarray(fg) != 0)
  return np.where(n > 0, n << 8 | tstar, 0).astype(np.uint16)


def paint(wmap, pos, colour, mutant=None):
  """uint8 [Kp,B,Hf,Wf,3]: picture k holds colour[b,k,t*] where n > pos[k], else 0.  colour uint8 [B,Kp,T,3].  mutant 'ge':
  n >= pos[k]."""
  B, Kp, T = colour.shape[:3]
  n, t = (wmap >> 8).astype(np.int64), (wmap & 255).astype(np.int64)
  out = np.zeros((Kp,) + wmap.shape + (3,), np.uint8)
  for k in range(Kp):
    on = (n >= pos[k]) if mutant == 'ge' else (n > pos[k])
    on = on & (t < T)
    for b in range(B):
      out[k, b] = colour[b, k][np.minimum(t[b], T - 1)] * on[b][..., None].astype(np.uint8)
  return out


def paint_gt(gt_ids, inst_id, colour):
  """uint8 [B,Hf,Wf,3]: the colour [B,T,3] of the first slot whose inst_id equals the pixel's id, 0 where there is none."""
  B, T = inst_id.shape
  j = ieo.slots(gt_ids, inst_id)
  out = np.zeros(gt_ids.shape + (3,), np.uint8)
  for b in range(B):
    out[b] = colour[b][np.minimum(j[b], T - 1)] * (j[b] < T)[..., None].astype(np.uint8)
  return out


def picture_from_masks(y, colour):
  """analysis.py:137-147 on masks y [B,T,Hf,Wf] with colour [B,T,3]: sum over t of uint8(y_t) * colour_t, in uint8."""
  B, T = y.shape[:2]
  img = np.zeros((B,) + y.shape[2:] + (3,), np.uint8)
  for b in range(B):
    for t in range(T):
      img[b] += y[b, t].astype(np.uint8)[..., None] * colour[b, t][None, None, :]
  return img


def picture_first(y, colour):
  """analysis.py:166-187 on planes y [B,T,Hf,Wf]: in the order t = 0 .. T - 1 a channel is written only while it is still 0."""
  B, T = y.shape[:2]
  img = np.zeros((B,) + y.shape[2:] + (3,), np.uint8)
  for b in range(B):
    for t in range(T):
      img[b] += (img[b] == 0) * (y[b, t].astype(np.uint8)[..., None] * colour[b, t][None, None, :])
  return img


def default_colours(T):
  """analysis.INSTANCE_CMAP[t % 22] in the picture's memory order (B, G, R): uint8 [T,3]."""
  import analysis
  cmap = np.array(analysis.INSTANCE_CMAP, np.uint8)
  return np.ascontiguousarray(cmap[np.arange(T) % cmap.shape[0]][:, ::-1])


def random_colours(seed, *shape):
  """uint8 shape + [3], no channel 0: a painted pixel is never black in any channel."""
  return np.random.RandomState(seed).randint(1, 256, tuple(shape) + (3,)).astype(np.uint8)


def keep_of(v, gt_ids, inst_id, thresholds, fg, tiny):
  """bool [B,K,T]: the predictions ins_eval_oracle.apply_remove_tiny leaves at each threshold."""
  inter, _ = ieo.counts(v, gt_ids, inst_id, thresholds, fg)
  return np.stack([ieo.apply_remove_tiny(inter[:, k], np.ones(inst_id.shape), tiny)[1] > 0 for k in range(len(thresholds))], axis=1)


def check_map_in_band(got, v, thresholds, fg=None, delta=ieo.DELTA):
  """The band rule of ins_eval_oracle on the map: a DECIDED pixel's word equals map_of's; an undecided pixel — its maximum m
  within delta of a threshold, or the runner-up within 2 delta of m while m could pass the lowest threshold — holds (t*, n) among
  its candidates: t* any instance within 2 delta of m, n between the thresholds below m - delta and those below m + delta (the
  word 0 where that range holds 0).  Returns the number of undecided pixels; raises AssertionError otherwise."""
  ref = map_of(v, thresholds, fg)
  thr = np.asarray(thresholds, np.float64)
  srt = np.sort(v, axis=1)
  m = srt[:, -1]
  second = srt[:, -2] if v.shape[1] > 1 else np.full_like(m, -np.inf)
  on = np.ones(m.shape, bool) if fg is None else np.asarray(fg) != 0
  near = (np.abs(m[..., None] - thr) <= delta).any(axis=-1)
  close = ((m - second) <= 2 * delta) & (m > thr.min() - delta)
  undecided = on & (near | close)
  assert (got[~undecided] == ref[~undecided]).all(), 'a decided pixel differs'
  gn, gt_ = (got >> 8).astype(np.int64), (got & 255).astype(np.int64)
  n_lo = ((m[..., None] - delta) > thr).sum(axis=-1)
  n_hi = ((m[..., None] + delta) > thr).sum(axis=-1)
  cand = np.take_along_axis(v, np.minimum(gt_, v.shape[1] - 1)[:, None], axis=1)[:, 0] >= m - 2 * delta
  ok = np.where(gn == 0, (got == 0) & (n_lo == 0), (gn >= n_lo) & (gn <= n_hi) & cand & (gt_ < v.shape[1]))
  assert ok[undecided].all(), 'an undecided pixel holds a word outside its candidates'
  return int(undecided.sum())


def inter_of_map(wmap, gt_ids, inst_id, pos):
  """inter int64 [B,K,T,T + 1] from the map's histogram joined with ins_eval_oracle.slots."""
  B, T = inst_id.shape
  j = ieo.slots(gt_ids, inst_id)
  n, t = (wmap >> 8).astype(np.int64), (wmap & 255).astype(np.int64)
  out = np.zeros((B, len(pos), T, T + 1), np.int64)
  for b in range(B):
    for k, pk in enumerate(pos):
      sel = n[b] > pk
      np.add.at(out[b, k], (t[b][sel], j[b][sel]), 1)
  return out
