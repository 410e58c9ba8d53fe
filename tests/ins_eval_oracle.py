"""Float64 NumPy restatement of the decode loop's evaluator at the labels' size, from instance-id images: the chain of the
reference's full_model_eval.py:97-139 behind apply_confidence — upsample (fg_eval_oracle.upsample: ra_oracle.pp_upsample with
the border rule written for size 1) [-> ra_oracle.pp_morph] -> ra_oracle.pp_apply_one_label -> per threshold
pp_apply_threshold [-> mask_foreground] — reduced to the counts ra_instance_eval_counts_f32 returns, the metrics of
ra_oracle.eval_metrics from those counts, and the BAND inside which a float32 evaluation of the same chain may fall.
The test helper of test_ins_eval*.py.

The band.  With DELTA = 1e-5 (the sweep test's bound on resize + bilateral in float32; the tree measures 2e-6) a pixel is
UNDECIDED at threshold k when |m - thr_k| <= DELTA (its maximum m may land on either side), or when m > thr_k - DELTA and
the runner-up is within 2 DELTA of m (another instance may win it).  lo counts the decided pixels only; hi adds every
undecided pixel to each (t, j) it could fall into: its ground-truth slot j is fixed, t is any instance within 2 DELTA of m.
The band is only a statement about the device when few pixels are undecided and no two instances tie EXACTLY at a maximum that
counts (an exact tie is decided by the order of the instances, which is checked on purpose-built inputs instead):
conditions() states both, and the tests assert them for every case — a condition on the inputs, not a tolerance."""
import numpy as np

import cs_oracle as cso
import fg_eval_oracle as fgo
import ra_oracle as ora

DELTA = 1e-5        # tests/test_fg_eval_gpu.py DELTA
BAND_SHARE = 1e-3   # tests/test_fg_eval_gpu.py BAND_SHARE: undecided pixels per image and threshold

# B, T, Hs, Ws, Hf, Wf, seed.  The first three have an EMPTY band (tests/test_ins_eval.py holds them to it), so the device's
# counts must equal the oracle's exactly; the next two exercise the band rule and the largest T.
MAIN_CASES = {
    'b2_t5_24x40_61x103': (2, 5, 24, 40, 61, 103, 1),
    'b1_t3_16x16_16x16': (1, 3, 16, 16, 16, 16, 3),
    'b2_t4_8x12_37x50': (2, 4, 8, 12, 37, 50, 4),
    'b1_t20_32x64_128x256': (1, 20, 32, 64, 128, 256, 2),
    'b1_t32_12x20_40x132': (1, 32, 12, 20, 40, 132, 5),
}
EMPTY_BAND = ('b2_t5_24x40_61x103', 'b1_t3_16x16_16x16', 'b2_t4_8x12_37x50')
# the smallest shapes at which the kernel takes another path: one pixel, down-sizing, a width that is no multiple of 4 (byte
# and word loads instead of vector loads), one pixel over the 16 x 128 tile in each direction (several tiles, several
# workgroups, a tile of one row and one of one column)
EDGE_CASES = {
    'b1_t1_1x1_1x4': (1, 1, 1, 1, 1, 4, 5),
    'b3_t2_4x4_2x3': (3, 2, 4, 4, 2, 3, 5),
    'b1_t3_6x9_19x30': (1, 3, 6, 9, 19, 30, 5),
    'b1_t2_5x33_17x129': (1, 2, 5, 33, 17, 129, 5),
    # Hf * Wf % 4 == 0, which the plane kernels of the chain (ra_postprocess_f32, ra_pair_stats_f32) need, with an empty band at
    # every K: the case on which the metrics from the counts are held to ops.eval_metrics on the chain's masks element for element
    'b2_t4_10x14_36x52': (2, 4, 10, 14, 36, 52, 9),
}
CASES = dict(MAIN_CASES, **EDGE_CASES)
THRESHOLDS = {1: [0.3],
              10: [0.5, 0.0, 0.9, 0.2, 0.7, 0.1, 0.8, 0.3, 0.6, 0.4],  # 0.0 .. 0.9 (full_model_eval.py:39-40), unsorted
              16: [0.45, 0.06, 0.9, 0.3, 0.3, 0.75, 0.0, 0.12, 0.6, 0.18, 0.84, 0.24, 0.54, 0.36, 0.66, 0.42]}  # with a repeat


def make_case(name):
  """{'yc' float32 [B,T,Hs,Ws], 'gt_ids' int32 [B,Hf,Wf], 'inst_id' int32 [B,T], 'fg' uint8 [B,Hf,Wf], 's_gt' float32 [B,T]}.
  yc: a smooth map per instance times a confidence in [0.3, 1].  gt_ids: discs painted over each other, ids from 1; the
  slots list them in a shuffled order with -1 slots in between, one slot names an id the image does not hold, and where
  the image holds more ids than slots remain those are listed by no slot."""
  B, T, Hs, Ws, Hf, Wf, seed = CASES[name]
  rng = np.random.RandomState(seed)
  y = fgo.smooth_map(rng, B * T, Hs, Ws).reshape(B, T, Hs, Ws)
  conf = rng.uniform(0.3, 1.0, (B, T)).astype(np.float32)
  yc = (y * conf[:, :, None, None]).astype(np.float32)
  rr, cc = np.mgrid[0:Hf, 0:Wf]
  n_disc = T + 2
  gt_ids = np.zeros((B, Hf, Wf), np.int32)
  inst_id = np.full((B, T), -1, np.int32)
  for b in range(B):
    for i in range(n_disc):
      cy, cx, rad = rng.uniform(0, Hf), rng.uniform(0, Wf), rng.uniform(0.1, 0.3) * max(2, min(Hf, Wf))
      gt_ids[b][(rr - cy) ** 2 + (cc - cx) ** 2 <= rad ** 2] = 7 * (i + 1)
    ids = list(rng.permutation(7 * (1 + np.arange(n_disc))))
    slots = rng.permutation(T)[:max(1, T - 1 - T // 4)]  # the other slots stay -1
    if len(slots) >= 2:
      ids[1] = 5  # an id the image does not hold (every painted id is a multiple of 7)
    for s, i in zip(sorted(slots), ids):
      inst_id[b, s] = i
  fg = (fgo.disc_labels(rng, B, Hf, Wf, n_disc=4) > 0).astype(np.uint8)
  return {'yc': yc, 'gt_ids': gt_ids, 'inst_id': inst_id, 'fg': fg, 's_gt': (inst_id >= 0).astype(np.float32)}


def dilate(v, reflect=False):
  """ra_oracle.pp_morph; reflect: the mutant that reflects the border into the window instead of ignoring it."""
  if not reflect:
    return ora.pp_morph(v)
  H, W = v.shape[-2:]
  ri, ci = fgo._reflect101(np.arange(-2, H + 2), H), fgo._reflect101(np.arange(-2, W + 2), W)
  pad = v[..., ri, :][..., :, ci]
  out = np.full(v.shape, -np.inf)
  for dy in range(5):
    for dx in range(5):
      out = np.maximum(out, pad[..., dy:dy + H, dx:dx + W])
  return out


def values(yc, Hf, Wf, morph=False, mutant=None):
  """v [B,T,Hf,Wf] float64: upsample, then the dilation when morph.  mutant 'morph_first': the dilation in front of the
  bilateral filter; 'reflect': the dilation with a reflected border; 'radius1': a 3 x 3 window."""
  B, T, Hs, Ws = yc.shape
  src = np.asarray(yc, np.float64).reshape(B * T, Hs, Ws)
  if morph and mutant == 'morph_first':
    # at equal size the resize inside upsample is the identity (source coordinate d, weight 0): what remains is the filter
    return fgo.upsample(ora.pp_morph(cso.resize_linear(src, Hf, Wf)), Hf, Wf).reshape(B, T, Hf, Wf)
  v = fgo.upsample(src, Hf, Wf).reshape(B, T, Hf, Wf)
  if morph and mutant == 'radius1':
    pad = np.pad(v, [(0, 0), (0, 0), (1, 1), (1, 1)], constant_values=-np.inf)
    return np.max([pad[..., dy:dy + Hf, dx:dx + Wf] for dy in range(3) for dx in range(3)], axis=0)
  return dilate(v, reflect=mutant == 'reflect') if morph else v


def slots(gt_ids, inst_id):
  """[B,Hf,Wf]: the first slot whose inst_id equals the pixel's id, T when there is none; negative inst_id match nothing."""
  B, T = inst_id.shape
  j = np.full(gt_ids.shape, T, np.int64)
  for b in range(B):
    for s in range(T - 1, -1, -1):
      if inst_id[b, s] >= 0:
        j[b][gt_ids[b] == inst_id[b, s]] = s
  return j


def gt_planes(gt_ids, inst_id):
  """y_gt [B,T,Hf,Wf] float32: the plane of slot j is where the id image holds inst_id[b,j]."""
  j = slots(gt_ids, inst_id)
  return (j[:, None] == np.arange(inst_id.shape[1])[None, :, None, None]).astype(np.float32)


def masks(v, thr, fg=None, mutant=None):
  """The chain's binary masks [B,T,Hf,Wf] at one threshold: pp_apply_one_label -> pp_apply_threshold [-> mask_foreground].
  mutant 'last_max': the last maximum takes the pixel; 'ge': >= in place of >."""
  B, T = v.shape[:2]
  if mutant == 'last_max':
    am = T - 1 - np.argmax(v[:, ::-1], axis=1)
    one = (am[:, None] == np.arange(T)[None, :, None, None]) * v
  else:
    one = ora.pp_apply_one_label(v)
  y = (one >= thr) if mutant == 'ge' else ora.pp_apply_threshold(one, thr)
  y = y.astype(np.float64)
  return y * (np.asarray(fg)[:, None] != 0) if fg is not None else y


def counts_of_masks(y, gt_ids, inst_id):
  """(inter [B,T,T + 1], area_b [B,T]) int64 of binary masks y [B,T,Hf,Wf] against the id image."""
  B, T = inst_id.shape
  j = slots(gt_ids, inst_id)
  inter = np.zeros((B, T, T + 1), np.int64)
  for b in range(B):
    for t in range(T):
      inter[b, t] = np.bincount(j[b][y[b, t] > 0], minlength=T + 1)
  area_b = np.stack([np.bincount(j[b].ravel(), minlength=T + 1)[:T] for b in range(B)]).astype(np.int64)
  return inter, area_b


def counts(v, gt_ids, inst_id, thresholds, fg=None, mutant=None):
  """(inter [B,K,T,T + 1], area_b [B,T]) int64 of the chain on v = values(...)."""
  per = [counts_of_masks(masks(v, th, fg, mutant), gt_ids, inst_id) for th in thresholds]
  return np.stack([p[0] for p in per], axis=1), per[0][1]


def band(v, gt_ids, inst_id, thresholds, fg=None, delta=DELTA):
  """(lo, hi [B,K,T,T + 1] int64, undecided [B,K] pixel counts, ties [B]): see the module's docstring.  ties: the pixels
  whose two largest values are EQUAL in float64 with a maximum above the lowest threshold (and fg set, when given)."""
  B, T, Hf, Wf = v.shape
  K = len(thresholds)
  j = slots(gt_ids, inst_id)
  on = np.ones((B, Hf, Wf), bool) if fg is None else np.asarray(fg) != 0
  srt = np.sort(v, axis=1)
  m = srt[:, -1]
  second = srt[:, -2] if T > 1 else np.full_like(m, -np.inf)
  tstar = np.argmax(v, axis=1)
  close = (m - second) <= 2 * delta
  cand = v >= (m - 2 * delta)[:, None]  # [B,T,Hf,Wf]: the instances that may win the pixel
  lo, hi = np.zeros((B, K, T, T + 1), np.int64), np.zeros((B, K, T, T + 1), np.int64)
  und = np.zeros((B, K), np.int64)
  for k, th in enumerate(thresholds):
    undecided = on & ((np.abs(m - th) <= delta) | ((m > th - delta) & close))
    decided = on & ~undecided & (m > th)
    und[:, k] = undecided.sum(axis=(1, 2))
    for b in range(B):
      np.add.at(lo[b, k], (tstar[b][decided[b]], j[b][decided[b]]), 1)
      hi[b, k] = lo[b, k]
      for t in range(T):
        sel = undecided[b] & cand[b, t]
        hi[b, k, t] += np.bincount(j[b][sel], minlength=T + 1)
  ties = (on & (m == second) & (m > min(thresholds))).sum(axis=(1, 2))
  return lo, hi, und, ties


def conditions(v, gt_ids, inst_id, thresholds, fg=None):
  """The band's conditions on the inputs -> (lo, hi, largest undecided share, exact ties); the caller asserts share <=
  BAND_SHARE and ties == 0."""
  lo, hi, und, ties = band(v, gt_ids, inst_id, thresholds, fg)
  return lo, hi, float(und.max()) / (v.shape[2] * v.shape[3]), int(ties.sum())


def apply_remove_tiny(inter, conf, threshold):
  """postprocess.py:109-136 on the counts of one threshold: inter [B,T,T + 1], conf [B,T] -> (inter, conf)."""
  if threshold == 0:
    return inter, conf
  keep = inter.sum(axis=2) > threshold
  return inter * keep[..., None], conf * keep


def metrics_from_counts(inter, area_b, s_gt):
  """ra_oracle.eval_metrics (analysis.py:370-787) from the counts of ONE threshold — inter [B,T,T + 1], area_b [B,T], s_gt
  [B,T] — in float64: the same keys.  The areas of the two unions are the sums of the areas: the predictions are disjoint
  after one-label, the instances of an id image by construction."""
  inter, area_b, s_gt = np.asarray(inter, np.float64), np.asarray(area_b, np.float64), np.asarray(s_gt, np.float64)
  B, T = s_gt.shape
  nz = lambda x: x + np.equal(x, 0)
  num_obj = np.maximum(s_gt.sum(axis=1), 1)
  count_gt = s_gt.sum(axis=1)
  A_all = inter.sum(axis=2)
  count_out = (A_all > 0).astype(np.float64)
  out = {k: np.zeros(B) for k in ('sbd', 'wt_cov', 'unwt_cov', 'fg_iou', 'fg_dice', 'avg_fp', 'avg_fn')}
  lists = {k: [] for k in ('avg_pr', 'avg_re', 'obj_pr', 'obj_re')}
  ious = []
  for ii in range(B):
    I, A, Bs, no = inter[ii, :, :T], A_all[ii], area_b[ii], int(num_obj[ii])
    card = A[:, None] + Bs[None, :]
    iou = I / nz(card - I)
    dice = 2 * I / nz(card)
    ious.append(iou)
    out['sbd'][ii] = min(dice.max(axis=1)[:no].mean(), dice.max(axis=0)[:no].mean())
    cov = iou.max(axis=0)
    out['wt_cov'][ii] = (cov * (Bs / nz(Bs.sum())))[:no].sum()
    out['unwt_cov'][ii] = (cov * (1 / num_obj[ii]))[:no].sum()
    fi, fa, fb = I.sum(), A.sum(), Bs.sum()
    out['fg_iou'][ii] = fi / nz(fa + fb - fi)
    out['fg_dice'][ii] = 2 * fi / nz(fa + fb)
    out['avg_fp'][ii] = (count_out[ii] * np.equal(iou.sum(axis=1), 0)).sum()
    out['avg_fn'][ii] = (s_gt[ii] * np.equal(iou.sum(axis=0), 0)).sum()
    pr, re = I.sum(axis=1) / nz(A), I.sum(axis=0) / nz(Bs)
    m_out, m_gt = (iou.max(axis=1) >= 0.5).astype(np.float64), (iou.max(axis=0) >= 0.5).astype(np.float64)
    for jj in range(T):
      if count_out[ii, jj] > 0:
        lists['avg_pr'].append(pr[jj])
        lists['obj_pr'].append(m_out[jj])
    for jj in range(int(count_gt[ii])):
      lists['avg_re'].append(re[jj])
      lists['obj_re'].append(m_gt[jj])
  d = count_out.sum(axis=1) - count_gt
  out.update(count_mse=d ** 2, count_acc=(d == 0).astype(np.float64), dic=d, dic_abs=np.abs(d), iou_pairwise=np.array(ious))
  out.update({k: np.array(v) for k, v in lists.items()})
  return out
