"""The evaluator's kernels (csrc/ra_eval.hip: post-processing, metrics, the in-graph augmentation) over their dimension space:
one table of rows, one set of float64 references, one table of bars.  The shape is tests/loss_train_cases.py's, and its pieces
(CONDITIONING, MARGIN, EXACT, Guarded, SENTINEL, to_dev, bits_of, guarded_only, _row) are reused.

Families (ROWS[family] is the list of rows; a row is a Row(family, name, p, what) with p its dimensions and options):

  post       ra_postprocess_f32        grid (ceil(HW/1024), B), four pixels per thread, s_hard by the first T threads of block 0
  union      ra_union_f32              the same grid
  wsum1      ra_weighted_sum_f32       the same grid
  tiny       ra_remove_tiny_f32        grid (ceil(HW/8192), B T), a grid-stride loop of float4 stores, in place
  dilate     ra_dilate_f32             one thread per pixel, the (2 R + 1)^2 window clipped to the image
  resize     ra_resize_linear_f32      one thread per pixel, the source coordinate in float32 (ra_resample.h)
  bilateral  ra_bilateral5_f32         one thread per pixel, 13 taps, BORDER_REFLECT_101; two rows through utils/postprocess.upsample
  metrics    ra_eval_metrics_f32       one 256-thread workgroup per image striding T*T; three rows through ra_ops.eval_metrics on masks
  transform  ra_random_transform_f32   grid (ceil(plane/2048), N), a grid-stride loop over the elements
  jitter     ra_colour_jitter_f32      64 workgroups per image always, two passes, partial sums in a workspace

inputs(row) draws the row's float32 inputs (seeded), reference(row) is the operation in float64 (oracle/ra_oracle.py's functions
wherever it has them; where it has only a composite — pp_upsample, eval_metrics on masks, colour_jitter in float64 only — the
restatement here is held to the oracle's by tests/test_eval_cases.py) and reference(row, 'float32') is the same computation in
float32: tests/test_eval_cases.py asserts on the host that it sits CONDITIONING inside every bar, that the input conditions hold,
that every launch choice the table is meant to reach is reached, and that one NumPy mutant per family is rejected by the row
built for it.  scores(row, ref, got) is the one table of bars: [(what, err, bar)], a row passes where every err < bar; an exact
quantity scores its number of differing elements against EXACT.  launch(row, x, dev) runs the C ABI into guarded, NaN-filled
outputs (the jitter's workspace too).  REJECTED[family] are the refused calls, each with its code.

  python tests/eval_cases.py             the kernels' largest error per row and quantity (needs an MI355X)
  python tests/eval_cases.py --measure   the float32 CPU run's largest error per quantity over the table (host only): what the
                                         measured bars below were derived from
"""
import collections
import functools
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, 'rec-attend-public_amd'), os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests')):
  if _p not in sys.path:
    sys.path.insert(0, _p)

import ra_oracle as ora  # noqa: E402
from loss_train_cases import (CONDITIONING, EXACT, E_INVALID, E_SHAPE, MARGIN, TOL_WSUM, Guarded, Row, SENTINEL, _absmax, _differ, _rel1,  # noqa: E402,F401
                              _row, bits_of, f32, failures, guarded_only, to_dev, worst_by_quantity)

E_WORKSPACE = -3
# ---- bars the tree already holds these quantities to (absolute)
TOL_METRICS = 1e-6   # the ratios of ra_eval_metrics_f32: tests/test_eval_gpu.py test_eval_metrics
TOL_UPSAMPLE = 2e-6  # resize + bilateral, and the bilateral filter alone: tests/test_eval_gpu.py test_postprocess
# TOL_WSUM (3e-6 of max(1, |ref| max)): the weighted sum, tests/loss_train_cases.py
# ---- measured bars: CONDITIONING times the float32 CPU run's largest error over the family's rows (--measure prints it), rounded
# up to one significant digit; absolute.  tests/test_eval_gpu.py's 2e-6 does not hold 8 times the float32 run at these rows (it
# does for the bilateral filter at both sigmas: 2.269e-07 at 16x17-sc0.1-smooth, and for upsample: 2.425e-07 at upsample-13x16-5x7).
TOL_RESIZE = 6e-6  # the float32 source coordinate at a non-integer ratio: measured 6.866e-07 at 13x16-5x7
TOL_JITTER = 1e-5  # RGB -> HSV -> RGB multiplies the hue's rounding by 6 s v: measured 1.171e-06 at hw40000-b3-corner2

NINF = float('-inf')
EVAL_RATIOS, EVAL_COUNTS = (0, 1, 2, 3, 4), (5, 6, 7, 8, 9, 10, 11, 12)  # columns of stats: RA_EVAL_SBD .. FG_DICE; FP .. COUNT_OUT
EVALI_RATIOS, EVALI_FLAGS = (2, 3), (0, 1, 4, 5)                          # rows of inst: PIX_PR, PIX_RE; OBJ_PR, OBJ_RE, HAS_OUT, IS_GT


def _cd(a, b):
  return -(-a // b)


# ---- the rows

POST_HW = (4, 1020, 1024, 1028)
POST_BT = [(1, 1), (3, 5), (2, 32), (1, 256)]
THRESH_NAME = {0.5: 'half', 0.0: 'zero', NINF: 'ninf'}


def _post_rows():
  rows = []
  for HW in POST_HW:
    for B, T in POST_BT:
      if T == 256 and HW not in (4, 1028):
        continue
      for fg in (0, 1):
        for uni in (0, 1):
          for th in (0.5, 0.0, NINF):
            rows.append(_row('post', 'hw%d-b%dt%d-%s%s-%s' % (HW, B, T, 'fg' if fg else 'nofg', '-uni' if uni else '', THRESH_NAME[th]), B=B, T=T, HW=HW, fg=fg,
                             uni=uni, shard=1, thresh=th, seed=len(rows)))
  rows.append(_row('post', 'hw1028-b3t5-fg-uni-half-noshard', 's_hard null', B=3, T=5, HW=1028, fg=1, uni=1, shard=0, thresh=0.5, seed=len(rows)))
  return rows


def _union_rows():
  return [_row('union', 'hw%d-t%d' % (HW, T), B=3, T=T, HW=HW, seed=k) for k, (HW, T) in enumerate((HW, T) for HW in POST_HW for T in (1, 5, 32))]


WSUM1_KINDS = ('onehot', 'general', 'zeros')


def _wsum1_rows():
  rows = []
  for HW in POST_HW:
    for T in (1, 5, 32):
      for kind in WSUM1_KINDS:
        rows.append(_row('wsum1', 'hw%d-t%d-%s' % (HW, T, kind), B=3, T=T, HW=HW, kind=kind, seed=len(rows)))
  return rows


TINY_HW = (4, 8188, 8192, 8196, 16388)


def _tiny_rows():
  rows = []
  for HW in TINY_HW:
    for conf in (1, 0):
      for size in ('below', 'equal', 'above'):
        rows.append(_row('tiny', 'hw%d-1-%s-%s' % (HW, size, 'conf' if conf else 'noconf'), B=1, T=1, HW=HW, conf=conf, size=size, seed=len(rows)))
      rows.append(_row('tiny', 'hw%d-6-%s' % (HW, 'conf' if conf else 'noconf'), B=2, T=3, HW=HW, conf=conf, size='all', seed=len(rows)))
  return rows


DILATE_HW = [(1, 1), (1, 7), (7, 1), (3, 3), (5, 5), (16, 16), (16, 17), (2, 130)]


def _dilate_rows():
  rows = []
  for H, W in DILATE_HW:
    for R in (0, 2, 16):
      for vals in ('bin', 'real'):
        rows.append(_row('dilate', '%dx%d-r%d-%s' % (H, W, R, vals), N=3, H=H, W=W, R=R, vals=vals, seed=len(rows)))
  return rows


RESIZE_SHAPES = [((8, 12), (8, 12)), ((8, 12), (16, 24)), ((5, 7), (13, 16)), ((13, 16), (5, 7)), ((1, 1), (4, 6)), ((1, 9), (3, 20)), ((6, 5), (1, 1)),
                 ((2, 2), (64, 64))]


def _resize_rows():
  return [_row('resize', '%dx%d-%dx%d' % (Hs, Ws, H, W), N=3, Hs=Hs, Ws=Ws, H=H, W=W, seed=k) for k, ((Hs, Ws), (H, W)) in enumerate(RESIZE_SHAPES)]


BILATERAL_HW = [(1, 1), (1, 2), (2, 2), (3, 3), (5, 5), (1, 9), (9, 1), (16, 16), (16, 17)]
BILATERAL_SIGMA = [(10.0, 10.0), (0.1, 10.0)]


def _bilateral_rows():
  rows = []
  for H, W in BILATERAL_HW:
    for sc, ss in BILATERAL_SIGMA:
      for vals in ('smooth', 'bin'):
        rows.append(_row('bilateral', '%dx%d-sc%g-%s' % (H, W, sc, vals), kind='plane', N=3, H=H, W=W, sc=sc, ss=ss, vals=vals, seed=len(rows)))
  for (Hs, Ws), (H, W) in [((5, 7), (13, 16)), ((13, 16), (5, 7))]:
    rows.append(_row('bilateral', 'upsample-%dx%d-%dx%d' % (Hs, Ws, H, W), 'utils/postprocess.upsample', kind='upsample', B=2, T=3, Hs=Hs, Ws=Ws, H=H, W=W,
                     sc=10.0, ss=10.0, seed=len(rows)))
  return rows


# the kinds of image of a metrics row: count_gt = T with the planted IoUs; no ground truth; no outputs; some of each; neither
METRICS_BT = [((1, 1), ('full',)), ((3, 5), ('full', 'nogt', 'noout')), ((2, 21), ('part', 'empty')), ((2, 32), ('full', 'nogt'))]
METRICS_NULLS = ('fg', 'a_in_fgb', 'b_in_fga', 'iou', 'inst')
METRICS_MASKS = [(1, 1, 2, 2), (2, 5, 6, 10), (1, 32, 8, 8)]


def _metrics_rows():
  rows = []
  for (B, T), kinds in METRICS_BT:
    rows.append(_row('metrics', 'b%dt%d' % (B, T), kind='tables', B=B, T=T, kinds=kinds, null='', seed=len(rows)))
  for null in METRICS_NULLS:
    rows.append(_row('metrics', 'b3t5-no-%s' % null, kind='tables', B=3, T=5, kinds=METRICS_BT[1][1], null=null, seed=len(rows)))
  for B, T, H, W in METRICS_MASKS:
    rows.append(_row('metrics', 'masks-b%dt%d-%dx%d' % (B, T, H, W), 'ra_ops.eval_metrics', kind='masks', B=B, T=T, H=H, W=W, null='', seed=len(rows)))
  return rows


TRANSFORM_HWC = [(1, 1, 1), (5, 7, 3), (16, 16, 8), (16, 16, 9), (16, 8, 16)]
TRANSFORM_PAD = 3


def transform_crops(H):
  """(padding, off_y, off_x, name)."""
  p = TRANSFORM_PAD
  return [(0, 0, 0, 'p0'), (p, 0, 0, 'p%d-0' % p), (p, p, p, 'p%d-mid' % p), (p, 2 * p, 2 * p - 1, 'p%d-far' % p), (H + 2, 0, 0, 'allpad')]


def _transform_rows():
  rows = []
  for H, W, C in TRANSFORM_HWC:
    for pad, oy, ox, cname in transform_crops(H):
      for tr in ((0, 1) if H == W else (0,)):
        for fv in (0, 1):
          for fh in (0, 1):
            rows.append(_row('transform', '%dx%dx%d-%s-v%dh%dt%d' % (H, W, C, cname, fv, fh, tr), N=2, H=H, W=W, C=C, pad=pad, oy=oy, ox=ox, fv=fv, fh=fh,
                             tr=tr, seed=len(rows)))
  return rows


JITTER_HW = (1, 255, 16384, 16385, 40000)
JITTER_DRAWS = [(0.0, 1.0, 0.0, 1.0), (0.1, 0.9, 0.1, 0.9), (0.1, 1.1, -0.1, 1.1), (-0.1, 0.9, -0.1, 1.1), (-0.1, 1.1, 0.1, 0.9)]  # hue, saturation, brightness, contrast


def _jitter_rows():
  rows = []
  for HW in JITTER_HW:
    for B in (1, 3):
      for d in range(len(JITTER_DRAWS)):
        rows.append(_row('jitter', 'hw%d-b%d-%s' % (HW, B, 'identity' if d == 0 else 'corner%d' % d), B=B, HW=HW, draw=d, seed=len(rows)))
  return rows


ROWS = collections.OrderedDict([('post', _post_rows()), ('union', _union_rows()), ('wsum1', _wsum1_rows()), ('tiny', _tiny_rows()), ('dilate', _dilate_rows()),
                                ('resize', _resize_rows()), ('bilateral', _bilateral_rows()), ('metrics', _metrics_rows()), ('transform', _transform_rows()),
                                ('jitter', _jitter_rows())])


def _rej(family, name, base, code, how, what=''):
  return _row(family, 'refuse-' + name, what, base=base, code=code, how=how)


# the refused calls: the arguments of the valid row `base` with one thing wrong (`how`), and the code the entry point returns
REJECTED = collections.OrderedDict([
    ('post', [_rej('post', 'hw15', 'hw1020-b3t5-fg-uni-half', E_SHAPE, 'hw15', 'H W = 3 x 5'),
              _rej('post', 'misaligned', 'hw1020-b3t5-fg-uni-half', E_SHAPE, 'misaligned', 'y_bin 4 bytes off a 16-byte boundary'),
              _rej('post', 't257', 'hw4-b1t256-fg-uni-half', E_SHAPE, 't257')]),
    ('union', [_rej('union', 'hw15', 'hw1020-t5', E_SHAPE, 'hw15'), _rej('union', 'misaligned', 'hw1020-t5', E_SHAPE, 'misaligned')]),
    ('wsum1', [_rej('wsum1', 'hw15', 'hw1020-t5-general', E_SHAPE, 'hw15'), _rej('wsum1', 'misaligned', 'hw1020-t5-general', E_SHAPE, 'misaligned')]),
    ('tiny', [_rej('tiny', 'hw15', 'hw8188-6-conf', E_SHAPE, 'hw15'), _rej('tiny', 'misaligned', 'hw8188-6-conf', E_SHAPE, 'misaligned')]),
    ('dilate', [_rej('dilate', 'r17', '16x17-r16-real', E_INVALID, 'r17'), _rej('dilate', 'inplace', '16x17-r2-real', E_INVALID, 'inplace')]),
    ('resize', []),
    ('bilateral', [_rej('bilateral', 'inplace', '16x17-sc10-smooth', E_INVALID, 'inplace'), _rej('bilateral', 'sigma0', '16x17-sc10-smooth', E_INVALID, 'sigma0'),
                   _rej('bilateral', 'sigma-nan', '16x17-sc10-smooth', E_INVALID, 'sigma-nan')]),
    ('metrics', [_rej('metrics', 't33', 'b2t32', E_SHAPE, 't33'), _rej('metrics', 'fg-inter-alone', 'b3t5', E_INVALID, 'fg-inter-alone', 'fg_inter without fg_a')]),
    ('transform', [_rej('transform', 'inplace', '16x16x8-p3-mid-v0h0t0', E_INVALID, 'inplace'),
                   _rej('transform', 'offset', '16x16x8-p3-far-v0h0t0', E_INVALID, 'offset', 'off_y = 2 padding + 1'),
                   _rej('transform', 'transpose', '16x8x16-p3-mid-v0h0t0', E_SHAPE, 'transpose', 'transpose with H != W')]),
    ('jitter', [_rej('jitter', 'short-ws', 'hw255-b3-corner1', E_WORKSPACE, 'short-ws', 'a workspace one float short')]),
])

ROW_OF = {(f, r.name): r for f, rs in ROWS.items() for r in rs}
ROW_OF.update({(f, r.name): r for f, rs in REJECTED.items() for r in rs})
FAMILY_SEED = {f: 7000000 + 100000 * k for k, f in enumerate(ROWS)}


def names(family):
  return [r.name for r in ROWS[family]]


def _rng(r, alt):
  return np.random.RandomState(FAMILY_SEED[r.family] + 10 * r.p['seed'] + (5 if alt else 0))


# ---- the launch choices, from the formulas of the C entry points (tests/test_eval_cases.py asserts what the table reaches)

def launch_choices(r):
  p = r.p
  if r.family in ('post', 'union', 'wsum1'):
    wg = _cd(p['HW'], 1024)
    c = dict(workgroups=wg, last_threads=_cd(p['HW'] - 1024 * (wg - 1), 4))
    if r.family == 'post':
      c['s_hard_threads'] = p['T'] if p['shard'] else 0
    return c
  if r.family == 'tiny':
    gx = _cd(p['HW'], 8192)
    return dict(workgroups=gx, passes=_cd(p['HW'] // 4, gx * 256), last_pass=p['HW'] // 4 - gx * 256 * (_cd(p['HW'] // 4, gx * 256) - 1))
  if r.family == 'dilate':
    return dict(workgroups=_cd(p['H'] * p['W'], 256), rows_in_window=min(p['H'], 2 * p['R'] + 1), cols_in_window=min(p['W'], 2 * p['R'] + 1),
                smaller_than_window=p['H'] < 2 * p['R'] + 1 or p['W'] < 2 * p['R'] + 1)
  if r.family == 'resize':
    ratio = lambda s, d: 'same' if s == d else 'one' if s == 1 else 'up-int' if d % s == 0 else 'up' if d > s else 'down'
    return dict(ratio_y=ratio(p['Hs'], p['H']), ratio_x=ratio(p['Ws'], p['W']), workgroups=_cd(p['H'] * p['W'], 256))
  if r.family == 'bilateral':
    return dict(workgroups=_cd(p['H'] * p['W'], 256), n_min=min(p['H'], p['W'], 5), n_max=min(max(p['H'], p['W']), 5))
  if r.family == 'metrics':
    TT = p['T'] * p['T']
    return dict(passes=_cd(TT, 256), last_pass=TT - 256 * (_cd(TT, 256) - 1), threads_live=p['T'])
  if r.family == 'transform':
    plane = p['H'] * p['W'] * p['C']
    gx = max(1, _cd(plane, 2048))
    return dict(plane=plane, workgroups=gx, passes=_cd(plane, gx * 256), last_pass=plane - gx * 256 * (_cd(plane, gx * 256) - 1))
  if r.family == 'jitter':
    HW = p['HW']
    return dict(passes=_cd(HW, 16384), last_pass=HW - 16384 * (_cd(HW, 16384) - 1), idle_workgroups=max(0, 64 - _cd(HW, 256)))
  raise KeyError(r.family)


# ---- inputs

def _away(a, centre):
  """a with every value closer than 2 MARGIN to centre pushed to 2 MARGIN from it."""
  a = np.array(a, dtype=np.float64)
  near = np.abs(a - centre) < 2 * MARGIN
  a[near] = centre + np.where(a[near] >= centre, 2, -2) * MARGIN
  return a


POST_TIE = 0.75  # the product every instance has at the tie pixel of image 0


def post_planted(r):
  """Pixels of image 0: (tie, zero, equal) — all T products exactly POST_TIE; all zero (every image has this one); the winner's
  product exactly thresh (thresh = 0: the zero pixel; -inf: none)."""
  HW, th = r.p['HW'], r.p['thresh']
  return HW - 1, 0, (1 if th == 0.5 else 0 if th == 0.0 else None)


def _post_inputs(r, alt):
  p, rng = r.p, _rng(r, alt)
  B, T, HW, th = p['B'], p['T'], p['HW'], p['thresh']
  s = f32(_away(rng.uniform(0.3, 1.0, (B, T)), 0.5))
  s[0] = rng.choice([1.0, 0.5, 0.25, 0.125], T)  # image 0: dyadic confidences, so products can be equal exactly in any precision
  s[0, 0] = 0.5                                  # exactly 0.5: not hard
  y = f32(rng.uniform(0.0, 0.9, (B, T, HW)))
  tie, zero, equal = post_planted(r)
  y[:, :, zero] = 0.0
  if equal == 1:
    y[0, :, 1] = np.float32(0.25) / s[0]
    y[0, T - 1, 1] = np.float32(th) / s[0, T - 1]
  y[0, :, tie] = np.float32(POST_TIE) / s[0]
  planted = np.zeros((B, HW), bool)
  planted[:, zero] = True
  planted[0, [tie] + ([1] if equal == 1 else [])] = True
  for _ in range(2):  # everywhere else: the two largest products MARGIN apart, the winner MARGIN from thresh
    prod = y.astype(np.float64) * s.astype(np.float64)[:, :, None]
    win = prod.argmax(axis=1)
    top = np.sort(prod, axis=1)[:, -2:]
    bump = np.zeros((B, HW))
    if T > 1:
      bump[top[:, 1] - top[:, 0] < 2 * MARGIN] = 3 * MARGIN
    if np.isfinite(th):
      bump[np.abs(top[:, -1] + bump - th) < 2 * MARGIN] += 4 * MARGIN
    bump[planted] = 0
    b_, q_ = np.nonzero(bump)
    y[b_, win[b_, q_], q_] += f32(bump[b_, q_] / s[b_, win[b_, q_]])
  x = {'y': y, 's': s}
  if p['fg']:
    fg = f32(rng.rand(B, HW) < 0.7)
    fg[0, tie] = 1.0
    fg[B - 1, HW // 2] = 0.0
    x['fg'] = fg
  return x


def _union_inputs(r, alt):
  p, rng = r.p, _rng(r, alt)
  y = f32(rng.randn(p['B'], p['T'], p['HW']))
  y[1] = f32(rng.rand(p['T'], p['HW']) > 0.7)  # one image of binary masks
  y[0, :, 0] = -np.abs(y[0, :, 0]) - np.float32(0.1)  # a pixel below zero in every plane
  y[2, 0, 1], y[2, 0, 2] = 5.0, -5.0                  # plane 0 the maximum, and (T > 1) not
  return {'y': y}


def wsum1_inf_plane(r, w):
  """(image, plane) of zero weight that holds an inf at pixel 2, or None: a skipped term is not evaluated."""
  T = r.p['T']
  if r.p['kind'] == 'general':
    return None
  if T == 1:
    return (1, 0) if r.p['kind'] == 'zeros' else None
  return 0, int(np.flatnonzero(w[0] == 0)[-1])


def _wsum1_inputs(r, alt):
  p, rng = r.p, _rng(r, alt)
  B, T, HW, kind = p['B'], p['T'], p['HW'], p['kind']
  if kind == 'onehot':
    w = np.zeros((B, T))
    w[np.arange(B), rng.randint(0, T, B)] = 1.0
  else:
    w = rng.randn(B, T)
    w[np.abs(w) < 0.05] = 0.05
    if kind == 'zeros':
      w[rng.rand(B, T) < 0.3] = 0.0
      w[1] = 0.0       # a row of zeros: the output is 0
      w[0, T - 1] = 0.0
      if T > 1:
        w[0, 0] = 0.7
  w, y = f32(w), f32(rng.rand(B, T, HW))
  at = wsum1_inf_plane(r, w)
  if at is not None:
    y[at[0], at[1], 2] = np.inf
  return {'w': w, 'y': y}


def tiny_threshold(HW):
  return float(max(2, int(round(0.375 * HW))))


def _tiny_plane(rng, HW, target):
  """HW values of {0, 1/4, 1/2, 3/4, 1} that add up to target exactly (in any precision: every partial sum is a multiple of 1/4 below 2^22)."""
  k = rng.randint(0, 5, HW)
  diff = int(round(target * 4)) - int(k.sum())
  for i in rng.permutation(HW):
    if diff == 0:
      break
    step = int(np.clip(diff, -k[i], 4 - k[i]))
    k[i] += step
    diff -= step
  assert diff == 0, (HW, target)
  return k / 4.0


def _tiny_inputs(r, alt):
  p, rng = r.p, _rng(r, alt)
  B, T, HW = p['B'], p['T'], p['HW']
  thr = tiny_threshold(HW)
  off = {'below': [-1], 'equal': [0], 'above': [1], 'all': [-1, 0, 1, 1, -1, 0]}[p['size']]
  if alt and p['size'] == 'all':
    off = off[::-1]
  y = f32([_tiny_plane(rng, HW, thr + o) for o in off]).reshape(B, T, HW)
  while alt and np.array_equal(y, _tiny_inputs(r, False)['y']):  # four pixels leave few planes to draw from
    y = f32([_tiny_plane(rng, HW, thr + o) for o in off]).reshape(B, T, HW)
  x = {'y': y, 'sizes': f32(y.astype(np.float64).sum(axis=2))}
  if p['conf']:
    x['conf'] = f32(rng.uniform(0.1, 0.9, (B, T)))
  return x


def _dilate_inputs(r, alt):
  p, rng = r.p, _rng(r, alt)
  shape = (p['N'], p['H'], p['W'])
  if p['vals'] == 'bin':
    y = f32(rng.rand(*shape) > 0.8)
    y[0] = 0.0
    y[0, p['H'] - 1, p['W'] - 1] = 1.0  # plane 0: one pixel, in the last corner
    if alt:
      y[1] = 1.0 - _dilate_inputs(r, False)['y'][1]
    return {'y': y}
  y = f32(rng.randn(*shape))
  y[1] = -np.abs(y[1]) - f32(0.1)  # a plane below zero everywhere: a border that counted as 0 would win
  return {'y': y}


def _resize_inputs(r, alt):
  p, rng = r.p, _rng(r, alt)
  return {'y': f32(rng.rand(p['N'], p['Hs'], p['Ws']))}


def _bilateral_inputs(r, alt):
  p, rng = r.p, _rng(r, alt)
  if p['kind'] == 'upsample':
    return {'y': f32(rng.rand(p['B'], p['T'], p['Hs'], p['Ws']))}
  N, H, W = p['N'], p['H'], p['W']
  if p['vals'] == 'bin':
    return {'y': f32(rng.rand(N, H, W) > 0.5)}
  rr, cc, nn = np.arange(H)[None, :, None], np.arange(W)[None, None, :], np.arange(N)[:, None, None]
  return {'y': f32(0.5 + 0.4 * np.sin(0.7 * rr + nn + (1.0 if alt else 0.0)) * np.cos(0.5 * cc) + 0.02 * rng.rand(N, H, W))}


METRICS_HALF, METRICS_NEAR = (0, 0), (1, 1)  # pairs of a 'full' image: IoU 200 / 400 exactly; 499 / 999


def _iou_int(i, a, b):
  u = a + b - i
  return i / u if u else 0.0


def _metrics_tables(r, alt):
  p, rng = r.p, _rng(r, alt)
  B, T = p['B'], p['T']
  I, A, Bs, sg = np.zeros((B, T, T)), np.zeros((B, T)), np.zeros((B, T)), np.zeros((B, T))
  for b, kind in enumerate(p['kinds']):
    n_gt = {'full': T, 'nogt': 0, 'noout': max(1, T // 2), 'part': max(1, T // 2), 'empty': 0}[kind]
    outs = {'full': np.arange(T), 'nogt': np.arange(max(1, T - 1)), 'noout': [], 'part': np.sort(rng.permutation(T)[:max(1, (2 * T) // 3)]), 'empty': []}[kind]
    sg[b, :n_gt] = 1.0
    Bs[b, :n_gt] = rng.randint(50, 4000, n_gt)
    A[b, outs] = rng.randint(50, 4000, len(outs))
    for i in outs:  # one overlap of a drawn IoU per output, a few small ones beside it
      for k, j in enumerate(rng.permutation(n_gt)[:3]):
        for _ in range(50):
          u = rng.uniform(0.05, 0.95) if k == 0 else rng.uniform(0.0, 0.05)
          v = min(int(u * (A[b, i] + Bs[b, j]) / (1 + u)), int(A[b, i]), int(Bs[b, j]))
          if abs(_iou_int(v, A[b, i], Bs[b, j]) - 0.5) >= 2 * MARGIN:
            break
        I[b, i, j] = v
    if kind == 'full':
      (i0, j0), (i1, j1) = METRICS_HALF, METRICS_NEAR
      A[b, i0], Bs[b, j0] = 300, 300
      I[b, i0, :], I[b, :, j0] = 0, 0
      I[b, i0, j0] = 200
      if T > 1:
        A[b, i1], Bs[b, j1] = 749, 749
        I[b, i1, :], I[b, :, j1] = 0, 0
        I[b, i1, j1] = 499
      if T > 3:
        I[b, 2, :] = 0  # an output that overlaps nothing: a false positive; a ground truth nothing overlaps: a false negative
        I[b, :, 3] = 0
  x = {'inter': f32(I), 'sum_a': f32(A), 'sum_b': f32(Bs), 's_gt': f32(sg)}
  fa, fb = A.sum(axis=1), Bs.sum(axis=1)
  x['fg_a'], x['fg_b'] = f32(fa), f32(fb)
  x['fg_inter'] = f32(np.floor(rng.uniform(0.2, 0.9, B) * np.minimum(fa, fb)))
  x['a_in_fgb'] = f32(np.floor(rng.uniform(0.0, 1.0, (B, T)) * (A + 1)).clip(0, A))
  x['b_in_fga'] = f32(np.floor(rng.uniform(0.0, 1.0, (B, T)) * (Bs + 1)).clip(0, Bs))
  return x


def _metrics_masks(r, alt):
  p, rng = r.p, _rng(r, alt)
  B, T, H, W = p['B'], p['T'], p['H'], p['W']
  n_gt = [max(1, T - 2)] + [max(0, T // 2 - 1)] * (B - 1)
  lab_out = rng.randint(0, T + 1, (B, H, W)) * (rng.rand(B, H, W) < 0.8)
  y_out = f32(lab_out[:, None] == np.arange(1, T + 1)[None, :, None, None])
  y_gt = np.zeros((B, T, H, W), np.float32)
  for b in range(B):
    lab = rng.randint(0, n_gt[b] + 1, (H, W))
    y_gt[b, :n_gt[b]] = lab[None] == np.arange(1, n_gt[b] + 1)[:, None, None]
  if T > 2:
    y_out[0, 1] = 0.0  # an instance without output
  return {'y_out': y_out, 'y_gt': y_gt, 's_gt': f32(np.arange(T)[None, :] < np.array(n_gt)[:, None])}


def _metrics_inputs(r, alt):
  return _metrics_masks(r, alt) if r.p['kind'] == 'masks' else _metrics_tables(r, alt)


def _transform_inputs(r, alt):
  p, rng = r.p, _rng(r, alt)
  return {'x': f32(rng.randn(p['N'], p['H'], p['W'], p['C']))}


JITTER_PLANTED = [(0.4, 0.4, 0.4), (0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (1.0, 1.0, 1.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (1.0, 1.0, 0.0), (0.3, 0.7, 0.7),
                  (0.7, 0.3, 0.7)]  # grey, black, red, white, green, blue, r == g == v, g == b == v, r == b == v


def _jitter_inputs(r, alt):
  p, rng = r.p, _rng(r, alt)
  B, HW = p['B'], p['HW']
  x = f32(rng.rand(B, HW, 3))
  for b in range(B):
    n = min(len(JITTER_PLANTED), HW)
    x[b, :n] = np.roll(np.array(JITTER_PLANTED, np.float32), -b - (3 if alt else 0), axis=0)[:n]  # HW = 1: grey, black, red by image
    if HW > 2 * len(JITTER_PLANTED):
      x[b, HW - 1] = JITTER_PLANTED[b % 3]  # the last pixel of the last pass
  return {'x': x}


_INPUTS = {'post': _post_inputs, 'union': _union_inputs, 'wsum1': _wsum1_inputs, 'tiny': _tiny_inputs, 'dilate': _dilate_inputs, 'resize': _resize_inputs,
           'bilateral': _bilateral_inputs, 'metrics': _metrics_inputs, 'transform': _transform_inputs, 'jitter': _jitter_inputs}


@functools.lru_cache(maxsize=None)
def _inputs_cached(family, name, alt):
  r = ROW_OF[(family, name)]
  if 'base' in r.p:  # a refused call: the inputs of the valid row it is derived from
    return _inputs_cached(family, r.p['base'], alt)
  x = _INPUTS[family](r, alt)
  for v in x.values():
    v.setflags(write=False)
  return x


def inputs(r, alt=False):
  """The row's float32 inputs (computed once per process, read-only); alt: another draw of the same shapes."""
  return _inputs_cached(r.family, r.name, bool(alt))


# ---- references

def post_explicit(r, x, dtype, last_max=False, ge_thresh=False):
  """recattend.h's statement: y_bin[b,t,p] = (t == argmax_t' y s) && (max_t' y s > thresh) [* fg], the FIRST maximum.  last_max,
  ge_thresh: the mutants (the last maximum wins; >= thresh)."""
  p = r.p
  B, T, HW = p['B'], p['T'], p['HW']
  yc, sh = ora.pp_apply_confidence(x['y'].astype(dtype).reshape(B, T, 1, HW), x['s'].astype(dtype))
  yc = yc.reshape(B, T, HW)
  assert yc.dtype == dtype
  am = (T - 1 - yc[:, ::-1].argmax(axis=1)) if last_max else yc.argmax(axis=1)
  top = yc.max(axis=1)
  keep = (top >= dtype(p['thresh'])) if ge_thresh else (top > dtype(p['thresh']))
  yb = (am[:, None, :] == np.arange(T)[None, :, None]) * keep[:, None, :].astype(np.float64)
  if 'fg' in x:
    yb = yb * x['fg'].astype(np.float64)[:, None, :]
  return yb, sh


def _post_reference(r, x, dtype, **mut):
  p = r.p
  B, T, HW = p['B'], p['T'], p['HW']
  if p['thresh'] >= 0 and not mut:  # the oracle's chain (above a negative threshold every non-winner's 0 would pass it)
    fg = x['fg'].astype(dtype).reshape(B, 1, HW) if 'fg' in x else None
    yb, sh = ora.postprocess(x['y'].astype(dtype).reshape(B, T, 1, HW), x['s'].astype(dtype), dtype(p['thresh']), fg=fg)
    yb = yb.reshape(B, T, HW)
  else:
    yb, sh = post_explicit(r, x, dtype, **mut)
  o = {'y_bin': yb}
  if p['shard']:
    o['s_hard'] = sh
  if p['uni']:
    o['union'] = yb.max(axis=1)
  return {k: np.asarray(v, dtype=np.float64) for k, v in o.items()}


def _union_reference(r, x, dtype, skip0=False):
  y = x['y'].astype(dtype)
  return {'union': (y[:, 1:] if skip0 and r.p['T'] > 1 else y).max(axis=1).astype(np.float64)}  # analysis.py:547,570


def _wsum1_reference(r, x, dtype, zero_as_one=False):
  w, y = x['w'].astype(dtype), x['y'].astype(dtype)
  if zero_as_one:
    w = np.where(w == 0, dtype(1), w)
  with np.errstate(invalid='ignore'):
    terms = np.where((w != 0)[:, :, None], w[:, :, None] * y, dtype(0))  # a zero weight's term is skipped, not multiplied
  out = terms.sum(axis=1)
  assert out.dtype == dtype
  return {'out': out.astype(np.float64)}


def _tiny_reference(r, x, dtype, keep_equal=False):
  p = r.p
  B, T, HW = p['B'], p['T'], p['HW']
  thr = tiny_threshold(HW) - (0.125 if keep_equal else 0.0)
  conf = x['conf'].astype(dtype) if 'conf' in x else np.ones((B, T), dtype)
  y, c = ora.pp_remove_tiny(x['y'].astype(dtype).reshape(B, T, 1, HW), conf, dtype(thr))
  o = {'y': y.reshape(B, T, HW)}
  if 'conf' in x:
    o['conf'] = c
  return {k: np.asarray(v, dtype=np.float64) for k, v in o.items()}


def dilate_ref(y, R, border=-np.inf):
  """ora.pp_morph for any radius: the maximum over the (2 R + 1)^2 window, pixels outside the image ignored."""
  H, W = y.shape[-2:]
  pad = np.pad(y, [(0, 0)] * (y.ndim - 2) + [(R, R), (R, R)], constant_values=border)
  out = np.full(y.shape, -np.inf, dtype=y.dtype)
  for dy in range(2 * R + 1):
    for dx in range(2 * R + 1):
      out = np.maximum(out, pad[..., dy:dy + H, dx:dx + W])
  return out


def _dilate_reference(r, x, dtype, zero_border=False):
  return {'out': dilate_ref(x['y'].astype(dtype), r.p['R'], 0.0 if zero_border else -np.inf).astype(np.float64)}


def resize_taps(n_src, n_dst, dtype, align_corners=False):
  """ora.pp_upsample's taps with the source coordinate evaluated in dtype, each operation rounded on its own: in float32 this is
  ra_resample.h's resize_linear_at ((float)n_src / (float)n_dst, (d + 0.5f) * scale - 0.5f, the fraction by subtraction)."""
  d = np.arange(n_dst).astype(dtype)
  if align_corners:
    f = d * dtype((n_src - 1) / max(n_dst - 1, 1))
  else:
    f = (d + dtype(0.5)) * (dtype(n_src) / dtype(n_dst)) - dtype(0.5)
  i0 = np.floor(f).astype(int)
  w = f - i0.astype(dtype)
  lo, hi = i0 < 0, i0 >= n_src - 1
  i0 = np.clip(i0, 0, n_src - 1)
  w = np.where(lo | hi, dtype(0), w)
  assert w.dtype == dtype
  return i0, np.minimum(i0 + 1, n_src - 1), w


def resize_ref(a, H, W, dtype, align_corners=False):
  a = a.astype(dtype)
  y0, y1, wy = resize_taps(a.shape[-2], H, dtype, align_corners)
  x0, x1, wx = resize_taps(a.shape[-1], W, dtype, align_corners)
  top = a[..., y0, :][..., :, x0] * (1 - wx) + a[..., y0, :][..., :, x1] * wx
  bot = a[..., y1, :][..., :, x0] * (1 - wx) + a[..., y1, :][..., :, x1] * wx
  out = top * (1 - wy)[:, None] + bot * wy[:, None]
  assert out.dtype == dtype
  return out


def reflect_index(i, n, mode='101'):
  """cv2's BORDER_REFLECT_101 (gfedcb|abcdefgh|gfedcba) or BORDER_REFLECT (fedcba|abcdefgh|hgfedcb) of the indices i into [0, n)."""
  i = np.array(i)
  if n == 1:
    return np.zeros_like(i)
  for _ in range(6):
    if mode == '101':
      i = np.where(i < 0, -i, i)
      i = np.where(i >= n, 2 * (n - 1) - i, i)
    else:
      i = np.where(i < 0, -i - 1, i)
      i = np.where(i >= n, 2 * n - 1 - i, i)
  assert ((i >= 0) & (i < n)).all()
  return i


def bilateral_ref(b, sigma_color, sigma_space, dtype, square=False, mode='101'):
  """ora.pp_upsample's bilateral step in dtype: gains -0.5 / sigma^2, one exponential of the summed exponent, 13 taps row by row."""
  b = b.astype(dtype)
  H, W = b.shape[-2:]
  gs, gc = dtype(-0.5) / (dtype(sigma_space) * dtype(sigma_space)), dtype(-0.5) / (dtype(sigma_color) * dtype(sigma_color))
  num, den = np.zeros_like(b), np.zeros_like(b)
  rr, cc = np.arange(H), np.arange(W)
  for dy in range(-2, 3):
    for dx in range(-2, 3):
      if dy * dy + dx * dx > 4 and not square:
        continue
      v = b[..., reflect_index(rr + dy, H, mode), :][..., :, reflect_index(cc + dx, W, mode)]
      wgt = np.exp(dtype(dy * dy + dx * dx) * gs + (v - b) * (v - b) * gc)
      num += wgt * v
      den += wgt
  out = num / den
  assert out.dtype == dtype
  return out


def _resize_reference(r, x, dtype, align_corners=False):
  return {'out': resize_ref(x['y'], r.p['H'], r.p['W'], dtype, align_corners).astype(np.float64)}


def _bilateral_reference(r, x, dtype, **mut):
  p = r.p
  if mut or dtype != np.float64:
    y = x['y'] if p['kind'] == 'plane' else resize_ref(x['y'], p['H'], p['W'], dtype)
    return {'out': bilateral_ref(y, p['sc'], p['ss'], dtype, **mut).astype(np.float64)}
  return {'out': ora.pp_upsample(x['y'], p['H'], p['W'], p['sc'], p['ss'])}  # at equal size its resize is the identity


def metrics_tables_of_masks(x, dtype):
  a, b = x['y_out'].astype(dtype), x['y_gt'].astype(dtype)
  ua, ub = a.max(axis=1), b.max(axis=1)
  s = lambda v: v.sum(axis=(-2, -1))
  return {'inter': np.einsum('bnhw,bmhw->bnm', a, b), 'sum_a': s(a), 'sum_b': s(b), 's_gt': x['s_gt'].astype(dtype), 'fg_inter': s(ua * ub), 'fg_a': s(ua),
          'fg_b': s(ub), 'a_in_fgb': s(a * ub[:, None]), 'b_in_fga': s(b * ua[:, None])}


def metrics_from_tables(t, dtype, null='', cov_other_axis=False, sbd_over_T=False):
  """ora.eval_metrics (analysis.py:314-787) from the intersections and sizes it computes of its masks, in dtype, laid out as
  ra_eval_metrics_f32's outputs: iou [B,T,T], stats [B,13] (RA_EVAL_*), inst [B,6,T] (RA_EVALI_*; the flags and ratios for every
  k, where the oracle lists only the k with an output / a ground truth)."""
  c = lambda k: np.asarray(t[k]).astype(dtype)
  I, A, Bs, sg = c('inter'), c('sum_a'), c('sum_b'), c('s_gt')
  B, T = A.shape
  uni, card = A[:, :, None] + Bs[:, None, :] - I, A[:, :, None] + Bs[:, None, :]
  iou = I / (uni + np.equal(uni, 0).astype(dtype))             # an_f_iou
  dice = 2 * I / (card + np.equal(card, 0).astype(dtype))      # _an_f_dice
  assert iou.dtype == dtype and dice.dtype == dtype
  stats, inst = np.zeros((B, 13)), np.zeros((B, 6, T))
  for b in range(B):
    count_gt = sg[b].sum()
    num_obj = max(count_gt, dtype(1))
    no = int(num_obj)
    has_out = (A[b] > 0).astype(dtype)
    bd_a, bd_b = dice[b].max(axis=1), dice[b].max(axis=0)
    sbd = min(bd_a[:no].sum() / dtype(T), bd_b[:no].sum() / dtype(T)) if sbd_over_T else min(bd_a[:no].mean(), bd_b[:no].mean())
    cov = iou[b].max(axis=1 if cov_other_axis else 0)
    tot = Bs[b].sum()
    wt = (cov * (Bs[b] / (tot + dtype(tot == 0))))[:no].sum()
    unwt = (cov * (dtype(1) / num_obj))[:no].sum()
    fp = (has_out * np.equal(iou[b].sum(axis=1), 0)).sum()
    fn = (sg[b] * np.equal(iou[b].sum(axis=0), 0)).sum()
    d = has_out.sum() - count_gt
    if null == 'fg':
      fg_iou = fg_dice = 0.0
    else:
      fi, fa, fb = c('fg_inter')[b], c('fg_a')[b], c('fg_b')[b]
      fu, fc = fa + fb - fi, fa + fb
      fg_iou, fg_dice = fi / (fu + dtype(fu == 0)), 2 * fi / (fc + dtype(fc == 0))
    stats[b] = [sbd, wt, unwt, fg_iou, fg_dice, fp, fn, float(d == 0), d * d, d, abs(d), num_obj, has_out.sum()]
    pa = c('a_in_fgb')[b] if null != 'a_in_fgb' else np.zeros(T, dtype)
    pb = c('b_in_fga')[b] if null != 'b_in_fga' else np.zeros(T, dtype)
    inst[b] = [iou[b].max(axis=1) >= 0.5, iou[b].max(axis=0) >= 0.5, pa / (A[b] + np.equal(A[b], 0)), pb / (Bs[b] + np.equal(Bs[b], 0)), has_out,
               np.arange(T) < count_gt]
  o = {'stats': stats}
  if null != 'iou':
    o['iou'] = iou.astype(np.float64)
  if null != 'inst':
    o['inst'] = inst
  return o


def _metrics_reference(r, x, dtype, **mut):
  t = metrics_tables_of_masks(x, dtype) if r.p['kind'] == 'masks' else x
  return metrics_from_tables(t, dtype, null=r.p['null'], **mut)


def _transform_reference(r, x, dtype, flips_after_transpose=False):
  p = r.p
  a = x['x'].astype(dtype)
  if flips_after_transpose and p['tr']:
    out = ora.random_transformation(a, p['pad'], p['oy'], p['ox'], False, False, True)
    out = out[:, ::-1] if p['fv'] else out
    out = out[:, :, ::-1] if p['fh'] else out
  else:
    out = ora.random_transformation(a, p['pad'], p['oy'], p['ox'], bool(p['fv']), bool(p['fh']), bool(p['tr']))
  return {'out': np.ascontiguousarray(out, dtype=np.float64)}


def jitter_ref(x, hue, saturation, brightness, contrast, dtype, one_mean=False):
  """ora.colour_jitter in dtype, operation for operation (csrc/ra_eval.hip's hue_sat_pixel in float32).  x [B,HW,3]."""
  f = dtype
  x = np.asarray(x).astype(f)
  r, g, b = x[..., 0], x[..., 1], x[..., 2]
  v = np.maximum(r, np.maximum(g, b))
  rng_ = v - np.minimum(r, np.minimum(g, b))
  s = np.where(v > 0, rng_ / np.where(v > 0, v, f(1)), f(0))
  with np.errstate(divide='ignore', invalid='ignore'):
    norm = f(1) / (f(6) * rng_)
    h = np.where(r == v, norm * (g - b), np.where(g == v, norm * (b - r) + f(2) / f(6), norm * (r - g) + f(4) / f(6)))
  h = np.where(rng_ > 0, h, f(0))
  h = np.where(h < 0, h + f(1), h)
  h = np.mod(h + (f(hue) + f(1)), f(1))
  s = np.clip(s * f(saturation), f(0), f(1))
  d6 = h * f(6)
  dr = np.clip(np.abs(d6 - f(3)) - f(1), f(0), f(1))
  dg = np.clip(f(2) - np.abs(d6 - f(2)), f(0), f(1))
  db = np.clip(f(2) - np.abs(d6 - f(4)), f(0), f(1))
  out = np.stack([(f(1) - s + s * dr) * v, (f(1) - s + s * dg) * v, (f(1) - s + s * db) * v], axis=-1) + f(brightness)
  # the means over the contiguous last axis: NumPy adds those pairwise (a strided axis it would add one after the other, 40000 long)
  mean = out.reshape(len(out), -1).mean(axis=1)[:, None, None] if one_mean else np.ascontiguousarray(out.transpose(0, 2, 1)).mean(axis=2)[:, None, :]
  out = (out - mean) * f(contrast) + mean
  assert out.dtype == dtype
  return out


def _jitter_reference(r, x, dtype, one_mean=False):
  p = r.p
  d = JITTER_DRAWS[p['draw']]
  if dtype == np.float64 and not one_mean:
    return {'out': ora.colour_jitter(x['x'].reshape(p['B'], 1, p['HW'], 3), *d).reshape(p['B'], p['HW'], 3)}
  return {'out': jitter_ref(x['x'], d[0], d[1], d[2], d[3], dtype, one_mean).astype(np.float64)}


_REFERENCE = {'post': _post_reference, 'union': _union_reference, 'wsum1': _wsum1_reference, 'tiny': _tiny_reference, 'dilate': _dilate_reference,
              'resize': _resize_reference, 'bilateral': _bilateral_reference, 'metrics': _metrics_reference, 'transform': _transform_reference,
              'jitter': _jitter_reference}


@functools.lru_cache(maxsize=None)
def _reference_cached(family, name, dtype):
  r = ROW_OF[(family, name)]
  out = _REFERENCE[family](r, inputs(r), getattr(np, dtype))
  for v in out.values():
    v.setflags(write=False)
  return out


def reference(r, dtype='float64'):
  """The row's reference, computed once per process and shared: callers leave it unchanged."""
  return _reference_cached(r.family, r.name, dtype)


# (dilate: a border reflected either way repeats pixels the window already holds, so it is the same maximum: the mutant is a border of 0)
MUTANTS = {'post': ('last-max', 'ge-thresh'), 'union': ('skip-plane0',), 'wsum1': ('zero-as-one',), 'tiny': ('lt',), 'dilate': ('zero-border',),
           'resize': ('align-corners',), 'bilateral': ('square', 'reflect'), 'metrics': ('cov-other-axis', 'sbd-over-T'), 'transform': ('flips-after-transpose',),
           'jitter': ('one-mean',)}


def mutant(r, which):
  """The reference with one plausible kernel error restated on it (float64), shaped like a kernel's result."""
  x, f = inputs(r), np.float64
  kw = {'last-max': dict(last_max=True), 'ge-thresh': dict(ge_thresh=True), 'skip-plane0': dict(skip0=True), 'zero-as-one': dict(zero_as_one=True),
        'lt': dict(keep_equal=True), 'zero-border': dict(zero_border=True), 'align-corners': dict(align_corners=True), 'square': dict(square=True),
        'reflect': dict(mode='reflect'), 'cov-other-axis': dict(cov_other_axis=True), 'sbd-over-T': dict(sbd_over_T=True),
        'flips-after-transpose': dict(flips_after_transpose=True), 'one-mean': dict(one_mean=True)}[which]
  assert which in MUTANTS[r.family], (r.family, which)
  with np.errstate(all='ignore'):
    return _REFERENCE[r.family](r, x, f, **kw)


# ---- scoring: [(what, err, bar), ...]; a row passes where every err < bar

def _bits_differ(got, ref32):
  got = np.ascontiguousarray(np.asarray(got), dtype=np.float32)
  assert got.shape == ref32.shape, (got.shape, ref32.shape)
  return int((got.view(np.int32) != np.ascontiguousarray(ref32).view(np.int32)).sum())


def scores(r, ref, got):
  p, x, out = r.p, inputs(r), []
  if r.family == 'post':
    for k in ('y_bin', 's_hard', 'union'):
      if k in ref:
        out.append((k, _differ(got[k], ref[k]), EXACT))
  elif r.family == 'union':
    out.append(('union', _differ(got['union'], ref['union']), EXACT))
  elif r.family == 'wsum1':
    out.append(('out', _rel1(got['out'], ref['out']), TOL_WSUM))
    zero = ~(x['w'] != 0).any(axis=1)
    out.append(('zero-weight images', int((np.asarray(got['out'])[zero] != 0).sum()), EXACT))
  elif r.family == 'tiny':
    out.append(('y', _differ(got['y'], ref['y']), EXACT))
    kept = x['sizes'] > tiny_threshold(p['HW'])
    out.append(('kept planes, bit for bit', _bits_differ(np.asarray(got['y'])[kept], x['y'][kept]), EXACT))
    if 'conf' in ref:
      out.append(('conf', _differ(got['conf'], ref['conf']), EXACT))
      out.append(('kept conf, bit for bit', _bits_differ(np.asarray(got['conf'])[kept], x['conf'][kept]), EXACT))
  elif r.family in ('dilate', 'transform'):
    out.append(('out', _differ(got['out'], ref['out']), EXACT))
  elif r.family == 'resize':
    out.append(('out', _absmax(got['out'], ref['out']), TOL_RESIZE))
    if (p['Hs'], p['Ws']) == (p['H'], p['W']):
      out.append(('copy, bit for bit', _bits_differ(got['out'], x['y']), EXACT))
  elif r.family == 'bilateral':
    out.append(('out', _absmax(got['out'], ref['out']), TOL_UPSAMPLE))
  elif r.family == 'metrics':
    st_g, st_r = np.asarray(got['stats']), ref['stats']
    if 'iou' in ref:
      out.append(('iou_pairwise', _absmax(got['iou'], ref['iou']), TOL_METRICS))
    out.append(('stats ratios', _absmax(st_g[:, EVAL_RATIOS], st_r[:, EVAL_RATIOS]), TOL_METRICS))
    out.append(('stats counts', _differ(st_g[:, EVAL_COUNTS], st_r[:, EVAL_COUNTS]), EXACT))
    if 'inst' in ref:
      in_g, in_r = np.asarray(got['inst']), ref['inst']
      out.append(('inst ratios', _absmax(in_g[:, EVALI_RATIOS], in_r[:, EVALI_RATIOS]), TOL_METRICS))
      out.append(('inst flags', _differ(in_g[:, EVALI_FLAGS], in_r[:, EVALI_FLAGS]), EXACT))
  elif r.family == 'jitter':
    out.append(('out', _absmax(got['out'], ref['out']), TOL_JITTER))
  return out


# ---- the input conditions (tests/test_eval_cases.py asserts them for every row)

def metrics_iou_margin(x):
  """The smallest distance from 0.5 of a constructed IoU, the exact 1/2 and the planted 499/999 left out."""
  I, A, Bs = (x[k].astype(np.float64) for k in ('inter', 'sum_a', 'sum_b'))
  uni = A[:, :, None] + Bs[:, None, :] - I
  iou = I / (uni + (uni == 0))
  d = np.abs(iou - 0.5)
  d[(I == 200) & (uni == 400)] = 1.0
  d[(I == 499) & (uni == 999)] = 1.0
  return float(d.min())


def conditions(r):
  """name -> bool, each a condition the row's inputs are meant to satisfy."""
  p, x, c = r.p, inputs(r), collections.OrderedDict()
  if r.family == 'post':
    B, T, HW, th = p['B'], p['T'], p['HW'], p['thresh']
    s = x['s'].astype(np.float64)
    prod = x['y'].astype(np.float64) * s[:, :, None]
    tie, zero, equal = post_planted(r)
    top = np.sort(prod, axis=1)[:, -2:]
    free = np.ones((B, HW), bool)
    free[:, zero] = False
    free[0, [tie] + ([1] if equal == 1 else [])] = False
    c['s: 0.5 exactly somewhere, MARGIN from it elsewhere'] = bool((s == 0.5).any() and np.abs(s[s != 0.5] - 0.5).min(initial=1) >= MARGIN)
    c['a full-T tie of exactly equal products above thresh'] = bool((prod[0, :, tie] == POST_TIE).all() and POST_TIE > th)
    c['the tie holds in float32'] = bool((x['y'][0, :, tie] * x['s'][0] == np.float32(POST_TIE)).all())
    c['an all-zero pixel in every image'] = bool((x['y'][:, :, zero] == 0).all())
    if equal is not None:
      c['a winner equal to thresh exactly'] = bool(prod[0, :, equal].max() == th and (x['y'][0, :, equal] * x['s'][0]).max() == np.float32(th))
    if T > 1:
      c['top two products MARGIN apart'] = bool((top[:, 1] - top[:, 0])[free].min(initial=1) >= MARGIN)
    if np.isfinite(th):
      c['winners MARGIN from thresh'] = bool(np.abs(top[:, -1] - th)[free].min(initial=1) >= MARGIN)
      c['winners on both sides of thresh'] = bool(HW < 16 or th == 0 or ((top[:, -1] > th).any() and (top[:, -1] < th).any()))
    if 'fg' in x:
      c['fg of zeros and ones, both present'] = bool(set(np.unique(x['fg'])) <= {0.0, 1.0} and x['fg'][0, tie] == 1 and (x['fg'] == 0).any())
  elif r.family == 'union':
    y = x['y']
    c['plane 0 holds the maximum somewhere, and not everywhere'] = bool(p['T'] == 1 or 0 < (y.argmax(axis=1) == 0).mean() < 1)
    c['pixels below zero in every plane'] = bool((y.max(axis=1) < 0).any())
  elif r.family == 'wsum1':
    w = x['w']
    at = wsum1_inf_plane(r, w)
    c['finite but for one planted inf under a zero weight'] = bool((~np.isfinite(x['y'])).sum() == (at is not None) and (at is None or w[at] == 0))
    if p['kind'] == 'onehot':
      c['one-hot'] = bool(((w == 1).sum(axis=1) == 1).all() and ((w == 0).sum(axis=1) == p['T'] - 1).all())
    if p['kind'] == 'zeros':
      c['an image of zero weights'] = bool((w[1] == 0).all())
      c['zeros among the other weights'] = bool(p['T'] == 1 or ((w[0] == 0).any() and (w[0] != 0).any()))
  elif r.family == 'tiny':
    thr = tiny_threshold(p['HW'])
    sz = x['y'].astype(np.float64).sum(axis=2).reshape(-1)
    want = {'below': {thr - 1}, 'equal': {thr}, 'above': {thr + 1}, 'all': {thr - 1, thr, thr + 1}}[p['size']]
    c['sizes below, equal to, one above the threshold'] = bool(set(sz) == want)
    c['the float32 sum is the size'] = bool(np.array_equal(x['y'].sum(axis=2, dtype=np.float32).reshape(-1), sz) and np.array_equal(x['sizes'].reshape(-1), sz))
    c['planes are dense'] = bool(p['HW'] < 64 or ((x['y'] != 0).mean(axis=2) > 0.5).all())
  elif r.family == 'dilate':
    y = x['y']
    if p['vals'] == 'bin':
      c['binary, plane 0 a single corner pixel'] = bool(set(np.unique(y)) <= {0.0, 1.0} and y[0].sum() == 1 and y[0, -1, -1] == 1)
    else:
      c['a plane below zero everywhere'] = bool((y[1] < 0).all())
  elif r.family == 'resize':
    c['in [0, 1)'] = bool(x['y'].min() >= 0 and x['y'].max() < 1)
  elif r.family == 'bilateral':
    y = x['y']
    c['in [0, 1]'] = bool(y.min() >= 0 and y.max() <= 1)
    if p['kind'] == 'plane' and p['vals'] == 'bin':
      c['binary'] = bool(set(np.unique(y)) <= {0.0, 1.0})
  elif r.family == 'metrics':
    if p['kind'] == 'tables':
      I, A, Bs, sg = (x[k].astype(np.float64) for k in ('inter', 'sum_a', 'sum_b', 's_gt'))
      c['whole numbers below 2^24'] = bool(all((x[k] == np.round(x[k])).all() and x[k].max() < 2 ** 24 and x[k].min() >= 0 for k in x))
      c['inter <= min(sum_a, sum_b)'] = bool((I <= np.minimum(A[:, :, None], Bs[:, None, :])).all() and (x['fg_inter'] <= np.minimum(x['fg_a'], x['fg_b'])).all()
                                             and (x['a_in_fgb'] <= x['sum_a']).all() and (x['b_in_fga'] <= x['sum_b']).all())
      c['s_gt a prefix of ones over the live ground truth'] = bool(((Bs > 0) == (sg > 0)).all() and (np.diff(sg, axis=1) <= 0).all())
      c['IoUs MARGIN from 0.5 but for the planted pair'] = metrics_iou_margin(x) >= MARGIN
      uni = A[:, :, None] + Bs[:, None, :] - I
      for b, kind in enumerate(p['kinds']):
        T = p['T']
        if kind == 'full':
          c['image %d: count_gt = T, IoU 1/2 exactly%s' % (b, ', 499/999' if T > 1 else '')] = bool(
              sg[b].sum() == T and I[b, 0, 0] * 2 == uni[b, 0, 0] and (I[b, 0, 1:] == 0).all() and (I[b, 1:, 0] == 0).all() and
              (T == 1 or (I[b, 1, 1] == 499 and uni[b, 1, 1] == 999)))
        if kind in ('nogt', 'empty'):
          c['image %d: count_gt = 0' % b] = bool(sg[b].sum() == 0 and Bs[b].sum() == 0)
        if kind in ('noout', 'empty'):
          c['image %d: no outputs' % b] = bool(A[b].sum() == 0)
        if kind in ('nogt', 'part'):
          c['image %d: both-empty pairs and live outputs' % b] = bool(((A[b][:, None] == 0) & (Bs[b][None, :] == 0)).any() and (A[b] > 0).any())
    else:
      t = metrics_tables_of_masks(x, np.float64)
      uni = t['sum_a'][:, :, None] + t['sum_b'][:, None, :] - t['inter']
      iou = t['inter'] / (uni + (uni == 0))
      c['IoUs 0.5 exactly or MARGIN from it'] = bool(np.abs(iou[iou != 0.5] - 0.5).min(initial=1) >= MARGIN)
      c['binary masks, one label per pixel'] = bool(x['y_out'].sum(axis=1).max() <= 1 and x['y_gt'].sum(axis=1).max() <= 1)
      c['N or M = 1 in the host chain: H W % 4 == 0'] = (p['H'] * p['W']) % 4 == 0
  elif r.family == 'transform':
    c['offsets within [0, 2 padding]'] = 0 <= p['oy'] <= 2 * p['pad'] and 0 <= p['ox'] <= 2 * p['pad']
    c['no element is zero'] = bool((x['x'] != 0).all())  # so a zero of the result is padding
    if p['pad'] - p['oy'] >= p['H']:
      c['the crop lies wholly in the padding'] = bool((reference(r)['out'] == 0).all())
  elif r.family == 'jitter':
    px = x['x'].reshape(-1, 3)
    mx, mn = px.max(axis=1), px.min(axis=1)
    c['a grey pixel'] = bool(((mx == mn) & (mx > 0)).any()) or p['HW'] == 1
    if p['HW'] >= len(JITTER_PLANTED):
      c['black, white, the primaries and the ties'] = bool((mx == 0).any() and (mn == 1).any() and all(
          ((px == np.array(q, np.float32)).all(axis=1)).any() for q in JITTER_PLANTED[2:]))
    else:
      c['planted pixels only'] = bool(all(any((q == np.array(k, np.float32)).all() for k in JITTER_PLANTED) for q in px))
    c['in [0, 1]'] = bool(px.min() >= 0 and px.max() <= 1)
  return c


# ---- the kernels through the C ABI (needs an MI355X)

def _ptr(t, off=0):
  return None if t is None else t.data_ptr() + off


def buffers(r, dev):
  """The row's guarded outputs."""
  p = r.p
  if r.family == 'post':
    B, T, HW = p['B'], p['T'], p['HW']
    bufs = {'y_bin': Guarded((B, T, HW), dev)}
    if p['shard']:
      bufs['s_hard'] = Guarded((B, T), dev)
    if p['uni']:
      bufs['union'] = Guarded((B, HW), dev)
    return bufs
  if r.family == 'union':
    return {'union': Guarded((p['B'], p['HW']), dev)}
  if r.family == 'wsum1':
    return {'out': Guarded((p['B'], p['HW']), dev)}
  if r.family == 'tiny':
    bufs = {'y': Guarded((p['B'], p['T'], p['HW']), dev)}
    if p['conf']:
      bufs['conf'] = Guarded((p['B'], p['T']), dev)
    return bufs
  if r.family in ('dilate', 'resize') or (r.family == 'bilateral' and p['kind'] == 'plane'):
    return {'out': Guarded((p['N'], p['H'], p['W']), dev)}
  if r.family == 'bilateral':
    return {}
  if r.family == 'metrics':
    if p['kind'] == 'masks':
      return {}
    B, T = p['B'], p['T']
    bufs = {'stats': Guarded((B, 13), dev)}
    if p['null'] != 'iou':
      bufs['iou'] = Guarded((B, T, T), dev)
    if p['null'] != 'inst':
      bufs['inst'] = Guarded((B, 6, T), dev)
    return bufs
  if r.family == 'transform':
    return {'out': Guarded((p['N'], p['H'], p['W'], p['C']), dev)}
  if r.family == 'jitter':
    return {'out': Guarded((p['B'], p['HW'], 3), dev), 'ws': Guarded((p['B'] * 64 * 3,), dev)}
  raise KeyError(r.family)


def call(r, xd, bufs, how=None):
  """The row's C entry point on the device inputs xd into bufs -> its return code.  how: one thing wrong (a REJECTED row's)."""
  import ra_native as rn
  L, st, p = rn.lib(), rn.stream_ptr(), r.p
  v = lambda k, off=0: _ptr(bufs[k].view, off) if k in bufs else None
  x = lambda k: _ptr(xd[k]) if k in xd else None
  mis = 4 if how == 'misaligned' else 0
  if r.family == 'post':
    B, T, HW = p['B'], p['T'], p['HW']
    H, W = (3, 5) if how == 'hw15' else (2, HW // 2)
    return L.ra_postprocess_f32(x('y'), x('s'), B, 257 if how == 't257' else T, H, W, p['thresh'], x('fg'), v('y_bin', mis), v('s_hard'), v('union'), st)
  if r.family == 'union':
    return L.ra_union_f32(x('y'), p['B'], p['T'], 15 if how == 'hw15' else p['HW'], v('union', mis), st)
  if r.family == 'wsum1':
    return L.ra_weighted_sum_f32(x('w'), x('y'), p['B'], p['T'], 15 if how == 'hw15' else p['HW'], v('out', mis), st)
  if r.family == 'tiny':
    return L.ra_remove_tiny_f32(v('y', mis), x('sizes'), v('conf'), p['B'], p['T'], 15 if how == 'hw15' else p['HW'], tiny_threshold(p['HW']), st)
  if r.family == 'dilate':
    return L.ra_dilate_f32(v('out') if how == 'inplace' else x('y'), p['N'], p['H'], p['W'], 17 if how == 'r17' else p['R'], v('out'), st)
  if r.family == 'resize':
    return L.ra_resize_linear_f32(x('y'), p['N'], p['Hs'], p['Ws'], p['H'], p['W'], v('out'), st)
  if r.family == 'bilateral':
    sc = {'sigma0': 0.0, 'sigma-nan': float('nan')}.get(how, p['sc'])
    return L.ra_bilateral5_f32(v('out') if how == 'inplace' else x('y'), p['N'], p['H'], p['W'], sc, p['ss'], v('out'), st)
  if r.family == 'metrics':
    null = p['null']
    fg = (None, None, None) if null == 'fg' else (x('fg_inter'), None if how == 'fg-inter-alone' else x('fg_a'), x('fg_b'))
    return L.ra_eval_metrics_f32(x('inter'), x('sum_a'), x('sum_b'), x('s_gt'), fg[0], fg[1], fg[2], None if null == 'a_in_fgb' else x('a_in_fgb'),
                                 None if null == 'b_in_fga' else x('b_in_fga'), p['B'], 33 if how == 't33' else p['T'], v('iou'), v('stats'), v('inst'), st)
  if r.family == 'transform':
    return L.ra_random_transform_f32(v('out') if how == 'inplace' else x('x'), p['N'], p['H'], p['W'], p['C'], p['pad'], p['oy'] + (1 if how == 'offset' else 0),
                                     p['ox'], p['fv'], p['fh'], 1 if how == 'transpose' else p['tr'], v('out'), st)
  if r.family == 'jitter':
    d = JITTER_DRAWS[p['draw']]
    n = bufs['ws'].n
    assert L.ra_colour_jitter_workspace_floats(p['B']) == n
    return L.ra_colour_jitter_f32(x('x'), p['B'], p['HW'], d[0], d[1], d[2], d[3], v('ws'), n - (1 if how == 'short-ws' else 0), v('out'), st)
  raise KeyError(r.family)


def refused(r, dev):
  """A REJECTED row -> (call, bufs, code): call() returns the entry point's code; bufs are the valid row's guarded outputs."""
  base = ROW_OF[(r.family, r.p['base'])]
  xd, bufs = to_dev({k: np.array(v) for k, v in inputs(base).items()}, dev), buffers(base, dev)  # copies: the cached inputs are read-only
  return (lambda: call(base, xd, bufs, how=r.p['how'])), bufs, r.p['code']


def launch(r, x, dev, bufs=None):
  """The row's kernels on inputs x into fresh guarded buffers (or bufs) -> (bufs, results shaped like reference()'s)."""
  import ra_native as rn
  xd, what, p = to_dev({k: np.array(v) for k, v in x.items()}, dev), '%s %s' % (r.family, r.name), r.p  # copies: the cached inputs are read-only
  if r.family == 'bilateral' and p['kind'] == 'upsample':
    from utils import postprocess as pp
    out = pp.upsample(xd['y'], torch.empty((p['B'], p['T'], p['H'], p['W']), dtype=torch.float32, device=dev))
    torch.cuda.synchronize()
    return {}, {'out': out.cpu().numpy()}
  if r.family == 'metrics' and p['kind'] == 'masks':
    import ra_ops
    m = ra_ops.eval_metrics(xd['y_out'], xd['y_gt'], xd['s_gt'])
    torch.cuda.synchronize()
    return {}, {'iou': m['iou_pairwise'].cpu().numpy(), 'stats': m['stats'].cpu().numpy(), 'inst': m['inst'].cpu().numpy()}
  bufs = bufs or buffers(r, dev)
  if r.family == 'tiny':  # in place: the planes and the confidences go into the guarded buffers first
    bufs['y'].view.copy_(xd['y'])
    if 'conf' in bufs:
      bufs['conf'].view.copy_(xd['conf'])
  if r.family == 'jitter':
    bufs['ws'].view.fill_(float('nan'))  # every record of the workspace must be written by this call
  rn.check(call(r, xd, bufs), what)
  got = {k: g.result('%s %s' % (what, k)) for k, g in bufs.items()}
  got.pop('ws', None)
  return bufs, got


def one_digit_up(v):
  """v rounded up to one significant digit."""
  if v <= 0:
    return 0.0
  e = math.floor(math.log10(v))
  return float('%.0e' % (math.ceil(v / 10 ** e - 1e-9) * 10 ** e))


def measure():
  """family -> {quantity: (largest error of the float32 CPU run, bar, row)}."""
  out = collections.OrderedDict()
  for family, rows in ROWS.items():
    worst = collections.OrderedDict()
    for r in rows:
      for w, e, bar in scores(r, reference(r), reference(r, 'float32')):
        key = w if not (family == 'bilateral' and r.p['kind'] == 'upsample') else 'upsample'
        if key not in worst or e > worst[key][0]:
          worst[key] = (e, bar, r.name)
    out[family] = worst
  return out


def main():
  import argparse
  ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
  ap.add_argument('--measure', action='store_true', help='the float32 CPU run of the reference against the float64 one (host only)')
  args = ap.parse_args()
  if args.measure:
    for family, worst in measure().items():
      for w, (e, bar, name) in worst.items():
        if bar == EXACT:
          print('%-9s %-26s float32 CPU run %d differ at %-34s (exact)' % (family, w, e, name), flush=True)
        else:
          print('%-9s %-26s float32 CPU run %.3e at %-34s bar %g (%.1f times inside; %g x the error, one digit up: %g)' % (
              family, w, e, name, bar, bar / e if e else np.inf, CONDITIONING, one_digit_up(CONDITIONING * e)), flush=True)
    return
  if not torch.cuda.is_available():
    raise SystemExit('eval_cases: needs an MI355X')
  dev = torch.device('cuda')
  worst = collections.OrderedDict()
  for family, rows in ROWS.items():
    for r in rows:
      sc = scores(r, reference(r), launch(r, inputs(r), dev)[1])
      for w, e, bar in sc:
        print(('%-9s %-36s %-26s %d differ  (exact)' % (family, r.name, w, e)) if bar == EXACT else
              ('%-9s %-36s %-26s %.3e  bar %g' % (family, r.name, w, e, bar)), flush=True)
        if bar != EXACT and e > worst.get((family, w), (-1.0,))[0]:
          worst[(family, w)] = (e, bar, r.name)
  for (family, w), (e, bar, name) in worst.items():
    print('worst %-9s %-26s %.3e at %s  bar %g' % (family, w, e, name, bar), flush=True)


if __name__ == '__main__':
  main()
