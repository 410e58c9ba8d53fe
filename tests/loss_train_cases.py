"""The loss side of the training step (csrc/ra_loss.hip and the loss-adjacent kernels of csrc/ra_train.hip) over its dimension
space: one table of rows, one set of float64 references, one table of bars.

Families (ROWS[family] is the list of rows; a row is a Row(family, name, p, what) with p its dimensions and options):

  head    ra_loss_head_f32 / ra_loss_head_bwd_f32   one 256-thread workgroup, four waves striding the images, 64 lanes striding T*T
  stats   ra_loss_stats_f32                         64 threads per image, red[16][32]
  wsum    ra_weighted_sum_multi[_strided]_f32       grid (ceil(HW/1024), N, B), four pixels per thread
  canvas  ra_canvas_step_f32                        grid (ceil(HW/256), B), the float4 group and lane of the canvas channel
  pair    ra_pair_stats[_strided]_f32               NI / NJ at N, M > 16, 4096-pixel chunks, the 8-way chunk reduction
  box     ra_gt_box_f32 -> ra_knob_setup_f32 -> ra_box_iou_rects_f32   8 slices per instance, TM at T <= 8 / 16, nblk <= 64

inputs(row) draws the row's float32 inputs (seeded), reference(row) restates the operation in float64 (NumPy, or torch on the CPU
where a gradient is taken by autograd; oracle/ra_oracle.py's functions wherever it has them) and reference(row, 'float32') is
the same computation in float32: tests/test_loss_train.py asserts on the host that it sits CONDITIONING inside every bar, that
the input conditions hold, that every launch choice the table is meant to reach is reached, and that one NumPy mutant per family
(a plausible kernel error restated on the reference) is rejected by the row built for it.  scores(row, ref, got) is the one
table of bars: [(what, err, bar)], a row passes where every err < bar; an exact quantity scores its number of differing
elements against EXACT.  launch(row, x, dev) runs the kernels through the C ABI into guarded, NaN-filled outputs.

  python tests/loss_train_cases.py             the kernels' largest error per row and quantity (needs an MI355X)
  python tests/loss_train_cases.py --measure   the float32 CPU run's largest error per quantity over the table (host only): what
                                               the measured bars below were derived from
"""
import collections
import functools
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, 'rec-attend-public_amd'), os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests')):
  if _p not in sys.path:
    sys.path.insert(0, _p)

import ra_oracle as ora  # noqa: E402
import ra_oracle_torch as orat  # noqa: E402
from ctrl_train_cases import CONDITIONING, TOL_GRAD, _per_image  # noqa: E402  (8.0; 2e-5 of the image's own |ref| max, no floor)

# ---- bars the tree already holds these quantities to
TOL_PAIR = 2e-5    # pairwise ratios and sums, of max(1, |ref| max): tests/test_loss_gpu.py test_pair_stats
TOL_PIECES = 2e-6  # loss pieces, of max(1, |ref|): tests/test_train_small_gpu.py test_loss_head_one_launch_equals_autograd_graph
# TOL_GRAD (2e-5): gradients and coefficient tensors, of the image's own |ref| max: tests/ctrl_train_cases.py
# ---- bars the tree has none for: CONDITIONING times the float32 CPU run's largest error over the table (--measure prints it),
# rounded up to one significant digit.  Each is per element, of max(1, |ref|), but for TOL_WSUM and TOL_RECT (of max(1, |ref| max)).
TOL_WSUM = 3e-6    # the weighted sum's output: measured 3.016e-07 at hw1024-n32t32-nobias
TOL_STATS = 2e-6   # the 12 real-valued statistics: measured 1.553e-07 (conf_loss) at b3t5-fixed-wtcov
TOL_BOX = 3e-6     # get_gt_box's corners: measured 2.861e-07 at 40x36-b8t8.  (tests/test_loss_gpu.py test_gt_box holds them to 1e-4
                   # absolute on maps of up to 128 x 128 with a whole-numbered padding; here the padding is a fraction and an empty
                   # or soft instance's corner lies near H W = 264192, where one float32 step is 0.03: the bar goes with the value,
                   # and is the tighter of the two for every coordinate below 33.)
TOL_CTR = 2e-6     # ra_knob_setup_f32's ctr: measured 2.187e-07 at 4x4-b8t8
TOL_SIZE = 5e-5    # ra_knob_setup_f32's size: measured 5.307e-06 at 516x512-b2t3 (shift * size and pad * size of an instance whose
                   # extent is H W / 2 pixels cancel in the difference)
TOL_RECT = 2e-6    # ra_box_iou_rects_f32's iou: measured 1.793e-07 at 40x36-b2t16
EXACT = 1          # an exact quantity scores its number of differing elements: fewer than one

MARGIN = 1e-3      # scores and a values from 0.5, scores from each other, rectangle corners from an integer, u from its threshold
E_SHAPE, E_INVALID = -2, -1

Row = collections.namedtuple('Row', 'family name p what')


def _row(family, name, what='', **p):
  return Row(family, name, collections.OrderedDict(sorted(p.items())), what)


def _head_rows():
  rows = []
  for (B, T), HW, mix, g, what in [
      ((1, 1), 16, 1.0, None, 'both loops of cum_ext are empty'),
      ((3, 5), 262144, 0.3, 0.7, 'fewer images than waves: the idle wave must still reach the barrier'),
      ((4, 8), 16, 0.0, None, 'T*T = 64: exactly one pass of the lanes; mix = 0'),
      ((5, 9), 262144, 1.0, 1.9, 'wave 0 takes a second image and reuses coef / idx; T*T = 81 leaves a ragged second pass'),
      ((2, 32), 16, 0.3, 0.7, 'the pipeline\'s maximum'),
      ((2, 64), 262144, 1.0, None, 'the ABI\'s maximum: every lane passes lane < T, T*T = 4096'),
      ((256, 2), 16, 0.3, 1.9, 'fills the last slot of per[]')]:
    rows.append(_row('head', 'b%dt%d' % (B, T), what, B=B, T=T, HW=HW, mix=mix, g=g, ties=False, seed=len(rows)))
  rows.append(_row('head', 'b3t5-ties', 'a repeated minimum, a repeated maximum, a run of 1.0f', B=3, T=5, HW=16, mix=1.0, g=None, ties=True, seed=20))
  rows.append(_row('head', 'b5t9-ties', 'the same where a wave takes two images', B=5, T=9, HW=262144, mix=0.3, g=1.9, ties=True, seed=21))
  return rows


HEAD_REJECTED = [_row('head', 'b257t2', 'B > 256', B=257, T=2, HW=16, mix=1.0, g=None, ties=False, seed=30),
                 _row('head', 'b2t65', 'T > 64', B=2, T=65, HW=16, mix=1.0, g=None, ties=False, seed=31)]


def _stats_rows():
  rows = []
  for B, T in [(1, 1), (3, 5), (2, 21), (5, 32)]:
    for fixed in (0, 1):
      for fn in (0, 1):
        rows.append(_row('stats', 'b%dt%d-%s-%s' % (B, T, 'fixed' if fixed else 'match', 'wtcov' if fn else 'iou'), B=B, T=T, fixed=fixed, fn=fn,
                         mix=0.3 if fn else 1.0, seed=len(rows)))
  return rows


def _wsum_rows():
  rows = []
  for HW in (4, 1020, 1024, 1028):
    for N, T in [(1, 1), (3, 5), (32, 32)]:
      for bias in (0, 1):
        rows.append(_row('wsum', 'hw%d-n%dt%d-%s' % (HW, N, T, 'bias' if bias else 'nobias'), B=3, HW=HW, N=N, T=T, bias=bias, seed=len(rows)))
  return rows


CANVAS_FORMS = ('nomatch', 'noise', 'nonoise')


def _canvas_rows():
  rows = []
  for HW in (255, 256, 257):
    for k, (C, cc) in enumerate([(4, 3), (4, 0), (8, 5), (12, 11)]):
      for form in CANVAS_FORMS:
        rows.append(_row('canvas', 'hw%d-c%dcc%d-%s' % (HW, C, cc, form), B=3, T=4, HW=HW, C=C, cc=cc, form=form, knob_stride=3 if k % 2 else 1,
                         seed=len(rows)))
  return rows


def _pair_rows():
  rows = []
  for N, M in [(1, 1), (16, 16), (17, 16), (16, 17), (17, 17), (32, 32)]:
    rows.append(_row('pair', 'n%dm%d-hw64' % (N, M), B=3, N=N, M=M, HW=64, seed=len(rows)))
  for HW in (4, 4092, 4096, 4100):
    rows.append(_row('pair', 'n17m17-hw%d' % HW, B=3, N=17, M=17, HW=HW, seed=len(rows)))
  rows.append(_row('pair', 'n2m2-hw36864', 'nine chunks: the 8-way unroll of the reduce kernel leaves a tail', B=3, N=2, M=2, HW=9 * 4096, seed=len(rows)))
  return rows


BOX_BT = [(1, 1), (8, 8), (5, 13), (2, 9), (2, 16), (2, 17), (1, 32)]


def _box_rows():
  rows = []
  for H, W in [(4, 4), (6, 4), (40, 36)]:
    for B, T in BOX_BT:
      rows.append(_row('box', '%dx%d-b%dt%d' % (H, W, B, T), B=B, T=T, H=H, W=W, seed=len(rows)))
  rows.append(_row('box', '9x4-b2t9', '36 pixels: slice 4 of the 8 is cut short by the end of the map', B=2, T=9, H=9, W=4, seed=len(rows)))
  for (H, W), (B, T), what in [((64, 64), (2, 9), 'nblk = 1'), ((64, 68), (2, 9), 'nblk = 2'),
                               ((516, 512), (2, 3), 'the smallest map at which the cap of 64 workgroups binds: a second pass each')]:
    rows.append(_row('box', '%dx%d-b%dt%d' % (H, W, B, T), what, B=B, T=T, H=H, W=W, seed=len(rows)))
  return rows


ROWS = collections.OrderedDict([('head', _head_rows()), ('stats', _stats_rows()), ('wsum', _wsum_rows()), ('canvas', _canvas_rows()),
                                ('pair', _pair_rows()), ('box', _box_rows())])
ROW_OF = {(f, r.name): r for f, rs in ROWS.items() for r in rs}
ROW_OF.update({(r.family, r.name): r for r in HEAD_REJECTED})
FAMILY_SEED = {f: 100000 * (k + 1) for k, f in enumerate(ROWS)}


def names(family):
  return [r.name for r in ROWS[family]]


def _rng(r, alt):
  return np.random.RandomState(FAMILY_SEED[r.family] + 10 * r.p['seed'] + (5 if alt else 0))


def f32(a):
  return np.ascontiguousarray(a, dtype=np.float32)


# ---- the launch choices, from the formulas of the C entry points (tests/test_loss_train.py asserts what the table reaches)

def launch_choices(r):
  p, cd = r.p, lambda a, b: -(-a // b)
  if r.family == 'head':
    TT = p['T'] * p['T']
    return dict(images_per_wave=cd(p['B'], 4), idle_waves=max(0, 4 - p['B']), passes=cd(TT, 64), last_pass=TT - 64 * (cd(TT, 64) - 1),
                lanes_live=min(p['T'], 64), last_slot=p['B'] - 1)
  if r.family == 'stats':
    return dict(rows_live=p['T'], workgroups=p['B'])
  if r.family == 'wsum':
    wg = cd(p['HW'], 1024)
    return dict(workgroups=wg, last_threads=cd(p['HW'] - 1024 * (wg - 1), 4))
  if r.family == 'canvas':
    wg = cd(p['HW'], 256)
    return dict(workgroups=wg, last_threads=p['HW'] - 256 * (wg - 1), group=p['cc'] >> 2, lane=p['cc'] & 3, groups=p['C'] // 4)
  if r.family == 'pair':
    nch = cd(p['HW'], 4096)
    return dict(NI=2 if p['N'] > 16 else 1, NJ=2 if p['M'] > 16 else 1, chunks=nch, chunks_mod8=nch % 8, last_chunk_px=p['HW'] - 4096 * (nch - 1))
  if r.family == 'box':
    HW, n = p['H'] * p['W'], p['B'] * p['T']
    per = cd(HW // 4, 8) * 4
    sizes = [max(0, min(HW, (s + 1) * per) - s * per) for s in range(8)]
    raw = cd(HW // 4, 1024)
    nblk = min(max(raw, 1), 64)
    return dict(slice_px=per, slices_empty=sizes.count(0), slices_short=sum(0 < s < per for s in sizes), TM=8 if p['T'] <= 8 else 16 if p['T'] <= 16 else 32,
                nblk=nblk, cap_binds=raw > 64, passes=cd(HW // 4, nblk * 256), workgroups=cd(n, 64), last_threads=n - 64 * (cd(n, 64) - 1))
  raise KeyError(r.family)


# ---- inputs

def _scores(rng, B, T, lo=0.02, hi=0.98):
  """[B, T] in (lo, hi), within an image pairwise more than MARGIN apart: a shuffled grid of 8 T cells, each score in the middle
  60 % of its cell (T = 64: cells of 1.9e-3)."""
  out = np.empty((B, T))
  for b in range(B):
    cells = rng.permutation(8 * T)[:T]
    out[b] = lo + (hi - lo) * (cells + 0.5 + rng.uniform(-0.2, 0.2, T)) / (8 * T)
  return out


def _partial_perm(rng, T, k, rows=None, cols=None):
  m = np.zeros((T, T), np.float32)
  rows = np.arange(T) if rows is None else rows
  cols = np.arange(T) if cols is None else cols
  m[rng.permutation(rows)[:k], rng.permutation(cols)[:k]] = 1.0
  return m


def _head_inputs(r, alt):
  p, rng = r.p, _rng(r, alt)
  B, T, HW = p['B'], p['T'], p['HW']
  x = {}
  for h in 'sb':  # masks / boxes: sums from 1e-6 HW (the 1e-5 HW term dominates the union) to HW / 2 (it is negligible)
    sa, sb = [f32(HW * 10.0 ** rng.uniform(-6, -0.3, (B, T))) for _ in range(2)]
    inter = f32(rng.uniform(0.05, 0.9, (B, T, T)) * np.minimum(sa[:, :, None], sb[:, None, :]))
    x['inter_' + h], x['sa_' + h], x['sb_' + h] = inter, sa, sb
    I, A, Bs = inter.astype(np.float64), sa.astype(np.float64)[:, :, None], sb.astype(np.float64)[:, None, :]
    x['iou_' + h] = f32(I / (A + Bs - I + 1e-5 * HW))
  ms, mb = np.zeros((B, T, T), np.float32), np.zeros((B, T, T), np.float32)
  for b in range(B):  # image 0 unmatched, image 1 fully matched by the masks, the others partly
    if B == 1:
      ks, kb = T, 0
    elif b == 0:
      ks, kb = 0, 0
    elif b == 1:
      ks, kb = T, int(rng.randint(1, T)) if T > 1 else 0
    else:
      ks, kb = int(rng.randint(1, T + 1)), int(rng.randint(0, T + 1))
    ms[b], mb[b] = _partial_perm(rng, T, ks), _partial_perm(rng, T, kb)
  x['m_s'], x['m_b'] = ms, mb
  if not p['ties']:
    x['s_out'] = f32(_scores(rng, B, T))
  else:
    s = f32(_scores(rng, B, T, 0.1, 0.9))
    s[0, [1, 3]] = 0.95   # image 0 (unmatched: only the maxima carry gradient): a repeated maximum
    s[1, [1, 3]] = 0.05   # image 1 (fully matched: only the minima do): a repeated minimum
    s[2, 1:4] = 1.0       # image 2 (partly matched): a run of 1.0f, what a saturated float32 sigmoid produces
    s[2, 0] = 0.05
    s[2, T - 1] = 0.05    # ... and a repeated minimum around it
    ms[2] = 0.0           # its matches: timestep 0 unmatched (its maximum is the run), the last one matched (its minimum repeats)
    ms[2, T - 1, 0] = ms[2, 2, 1] = 1.0
    if B > 4:             # the wave's second image: both kinds at once
      s[4, [2, 5]] = 0.05
      s[4, [0, 7]] = 0.95
    x['s_out'] = s
  if p['g'] is not None:
    x['g'] = f32([p['g']])
  return x


def _stats_inputs(r, alt):
  p, rng = r.p, _rng(r, alt)
  B, T = p['B'], p['T']
  n_gt = [int(rng.randint(max(1, T // 2), T + 1)) for _ in range(B)]
  if B >= 2:
    n_gt[0] = 0  # an image with no ground truth: s_gt, sum_gt and every IoU column zero
  s_gt = f32(np.arange(T)[None, :] < np.array(n_gt)[:, None])
  x = {'s_gt': s_gt, 'sum_gt': f32(s_gt * rng.randint(1, 4000, (B, T)))}
  for k in ('iou_soft', 'iou_hard', 'dice', 'iou_box'):  # an absent ground truth overlaps nothing
    x[k] = f32(rng.uniform(0.01, 0.99, (B, T, T)) * s_gt[:, None, :])
  mr, mb = np.zeros((B, T, T), np.float32), np.zeros((B, T, T), np.float32)
  for b in range(B):
    live = np.arange(n_gt[b])
    if n_gt[b] == 0 or (B >= 3 and b == 1):  # image 1: ground truth, but no match
      continue
    mr[b] = _partial_perm(rng, T, int(rng.randint(1, n_gt[b] + 1)), live, live)
    for _ in range(100):
      mb[b] = _partial_perm(rng, T, int(rng.randint(1, n_gt[b] + 1)), live, live)
      if n_gt[b] == 1 or not np.array_equal(mb[b], mr[b]):
        break
  x['match_real'], x['match_box'] = mr, mb
  s = _scores(rng, B, T)
  near = np.abs(s - 0.5) < 2 * MARGIN
  s[near] = 0.5 + np.where(s[near] >= 0.5, 2, -2) * MARGIN
  s = f32(s)
  s[B - 1, T // 2] = 0.5  # exactly 0.5: not counted
  x['s_out'] = s
  return x


def _wsum_inputs(r, alt):
  p, rng = r.p, _rng(r, alt)
  B, N, T, HW = p['B'], p['N'], p['T'], p['HW']
  w = rng.randn(B, N, T)
  w[np.abs(w) < 0.05] = 0.05
  if T > 1:
    w[rng.rand(B, N, T) < 0.2] = 0.0  # exact zeros among the weights: skipped terms
  w[1, 0, :] = 0.0  # a row of zeros: the output is the bias, bit for bit
  x = {'w': f32(w), 'y': f32(rng.rand(B, T, HW))}
  if p['bias']:
    x['bias'] = f32(rng.randn(B, N))
  return x


def _canvas_inputs(r, alt):
  p, rng = r.p, _rng(r, alt)
  B, T, HW, C = p['B'], p['T'], p['HW'], p['C']
  x = {'prev': f32(rng.rand(B, HW, C)), 'y': f32(rng.rand(B, HW))}
  if p['form'] != 'nomatch':
    m = np.zeros((B, T), np.float32)
    m[0, 2] = 1.0                  # one-hot; image 1: all zero; image 2: two fractional weights
    m[2, [0, 3]] = [0.25, 0.6]
    x['match'], x['y_gt'] = m, f32(rng.rand(B, T, HW) > 0.5)
    knob = f32(rng.rand(B, p['knob_stride']))
    knob[:, 0] = [0.0, 1.0, 0.37]
    x['knob'] = knob
    if p['form'] == 'noise':
      x['noise'] = f32(0.3 * rng.rand(B, HW))
  return x


def _pair_inputs(r, alt):
  p, rng = r.p, _rng(r, alt)
  B, N, M, HW = p['B'], p['N'], p['M'], p['HW']
  a = rng.rand(B, N, HW) ** 2
  near = np.abs(a - 0.5) < 2 * MARGIN
  a[near] = 0.5 + np.where(a[near] >= 0.5, 2, -2) * MARGIN
  a = f32(a)
  flat = a.reshape(-1)
  flat[rng.permutation(flat.size)[:min(5, flat.size // 2)]] = 0.5  # a handful exactly 0.5: not hard
  b = f32(rng.rand(B, M, HW) > 0.7)
  b[2] *= f32(rng.rand(M, HW))  # one image with a soft b
  a[0, N - 1], b[0, 0] = 0.0, 0.0  # an empty a plane, an empty b plane
  return {'a': a, 'b': b}


BOX_PAD_RATIO, BOX_MIN_PAD = 0.13, 2.3
BOX_KINDS = ('corner', 'empty', 'borders', 'soft', 'left')  # instance i of the flattened [B T] takes kind i where i < 5, then rectangles
KNOB_SCHED = (0.4, 0.7)


def _box_inputs(r, alt):
  p, rng = r.p, _rng(r, alt)
  B, T, H, W = p['B'], p['T'], p['H'], p['W']
  y = np.zeros((B * T, H, W), np.float32)
  for i in range(B * T):
    kind = BOX_KINDS[i] if i < len(BOX_KINDS) else 'rect'
    if kind == 'corner':
      y[i, H - 1, W - 1] = 1.0  # one pixel, the last of the last slice
    elif kind == 'borders':
      y[i, 0:2, W - 2:W] = 1.0
    elif kind == 'left':
      y[i, H // 2, 0] = 1.0
    elif kind in ('soft', 'rect'):
      for _ in range(1 if kind == 'soft' else 2):  # rect: the union of two
        y0, x0 = int(rng.randint(0, H)), int(rng.randint(0, W))
        y[i, y0:y0 + int(rng.randint(1, max(2, H // 3))), x0:x0 + int(rng.randint(1, max(2, W // 3)))] = 0.5 if kind == 'soft' else 1.0
  n = B * T
  x = {'y_gt': y.reshape(B, T, H, W), 'map': f32(rng.rand(B, H, W)), 'pad': f32(0.1 + 0.2 * rng.rand(B, T)), 'shift': f32(rng.uniform(-0.05, 0.05, (B, T, 2))),
       'sched': f32(KNOB_SCHED)}
  thr = knob_thresholds(T, p['seed'] % 2)
  for k, key in enumerate(('u_box', 'u_segm')):
    u = rng.rand(B, T)
    t = np.broadcast_to(thr[k], (B, T))
    near = np.abs(u - t) < 2 * MARGIN
    u[near] = np.clip(t[near] + np.where(u[near] >= t[near], 2, -2) * MARGIN, 0.0, 1.0)
    u[(u > 1 - 2 * MARGIN) & (t >= 1)] = 0.9  # under a threshold of 1 every draw passes: keep the margin all the same
    x[key] = f32(u)
  assert n == x['pad'].size
  return x


def knob_thresholds(T, timescale, dtype=np.float64):
  """[2, T]: min(sched[k] * scale_t, 1), scale_t = 1 + log(1 + 3 t) with the timescale (full_model.py:596-625)."""
  scale = (1.0 + np.log(1.0 + np.arange(T, dtype=dtype) * 3.0)) if timescale else np.ones(T, dtype)
  return np.minimum(np.asarray(KNOB_SCHED, dtype)[:, None] * scale[None, :], 1.0)


_INPUTS = {'head': _head_inputs, 'stats': _stats_inputs, 'wsum': _wsum_inputs, 'canvas': _canvas_inputs, 'pair': _pair_inputs, 'box': _box_inputs}


def inputs(r, alt=False):
  """The row's float32 inputs; alt: another draw of the same shapes (what a relaunch test fills the buffers with first)."""
  return _INPUTS[r.family](r, alt)


# ---- references

def cum_ext_indices(s, first_min=False):
  """imin[t], imax[t] of one image's scores: the LAST position of the minimum of s[0..t] and the SMALLEST index >= t holding the
  maximum of s[t..T) — what torch.cummin and flip(cummax(flip)) report on the CPU, and recattend.h documents.  first_min = True
  is the other choice (the first minimum, the largest index of the maximum): the routing of tf.minimum / tf.maximum chains."""
  T = len(s)
  imin, imax = np.zeros(T, int), np.zeros(T, int)
  for t in range(T):
    lo, hi = s[:t + 1].min(), s[t:].max()
    at_lo, at_hi = np.flatnonzero(s[:t + 1] == lo), t + np.flatnonzero(s[t:] == hi)
    imin[t], imax[t] = (at_lo[0], at_hi[-1]) if first_min else (at_lo[-1], at_hi[0])
  return imin, imax


def head_ds(x, p, dtype, first_min=False, coef_of=None):
  """d loss / d s_out by the explicit index rule.  coef_of(b): the image whose two coefficient rows image b adds up (a mutant's)."""
  B, T = p['B'], p['T']
  s, ms = x['s_out'].astype(dtype), x['m_s'].astype(dtype).sum(axis=2)
  k = dtype((p['g'] if p['g'] is not None else 1.0)) * dtype(p['mix']) / dtype(B) / dtype(T)
  eps = dtype(1e-5)
  ds = np.zeros((B, T), dtype)
  for b in range(B):
    imin, imax = cum_ext_indices(s[b], first_min)
    src = b if coef_of is None else coef_of(b)
    jmin, jmax = cum_ext_indices(s[src], first_min)
    for t in range(T):
      ds[b, imin[t]] += -k * ms[src, t] / (s[src, jmin[t]] + eps)
      ds[b, imax[t]] += k * (dtype(1) - ms[src, t]) / (dtype(1) - s[src, jmax[t]] + eps)
  return ds


def _head_reference(r, x, dtype, clamp=True):
  p = r.p
  B, T, HW = p['B'], p['T'], p['HW']
  td = getattr(torch, dtype)
  t = lambda a: torch.from_numpy(np.asarray(a)).to(td)
  m_s, m_b = t(x['m_s']), t(x['m_b'])

  def matched(iou, m):  # mean over the images of sum(iou m) / max(sum m, 1)
    cnt = m.sum(dim=(1, 2))
    return ((iou * m).sum(dim=(1, 2)) / (torch.clamp(cnt, min=1.0) if clamp else cnt)).sum() / B

  def conf_of(s):
    s_min = torch.cummin(s, dim=1)[0]
    s_max = torch.flip(torch.cummax(torch.flip(s, [1]), dim=1)[0], [1])
    ms = m_s.sum(dim=2)
    return (-ms * torch.log(s_min + 1e-5) - (1 - ms) * torch.log(1 - s_max + 1e-5)).sum() / B / T

  i_s, i_b, conf = matched(t(x['iou_s']), m_s), matched(t(x['iou_b']), m_b), conf_of(t(x['s_out']))
  n = lambda v: v.detach().to(torch.float64).numpy()
  out = {'pieces': np.array([float(v) for v in (-i_b - i_s + p['mix'] * conf, -i_b, -i_s, conf, i_s, i_b)])}
  # backward: the loss as a function of the raw intersections and sums (PairIoU's adjoint: c1 = d loss / d inter, c0 = d loss / d sum_a)
  leaves, ious = {}, {}
  for h in 'sb':
    I, sa = t(x['inter_' + h]).requires_grad_(True), t(x['sa_' + h]).requires_grad_(True)
    leaves[h] = (I, sa)
    ious[h] = I / (sa[:, :, None] + t(x['sb_' + h])[:, None, :] - I + 1e-5 * HW)
  s = t(x['s_out']).requires_grad_(True)
  loss = -matched(ious['b'], m_b) - matched(ious['s'], m_s) + p['mix'] * conf_of(s)
  g = p['g'] if p['g'] is not None else 1.0
  got = torch.autograd.grad(loss * g, [leaves['s'][0], leaves['s'][1], leaves['b'][0], leaves['b'][1], s], allow_unused=True)
  for key, v, like in zip(('c1_s', 'c0_s', 'c1_b', 'c0_b', 'ds_autograd'), got, (x['m_s'], x['sa_s'], x['m_b'], x['sa_b'], x['s_out'])):
    out[key] = np.zeros(like.shape) if v is None else n(v)
  # the tie rows: the index rule, explicit (torch's choice among equal scores is documented nowhere; the CPU's is the rule above)
  out['ds'] = head_ds(x, p, np.dtype(dtype).type).astype(np.float64) if p['ties'] else out['ds_autograd']
  return out


def _stats_reference(r, x, dtype):
  p = r.p
  B, T = p['B'], p['T']
  c = lambda k: x[k].astype(dtype)
  s_gt, s_out = c('s_gt'), c('s_out')
  ident = ora.get_identity_match(s_gt)
  real = c('match_real')
  match, match_box = (ident, ident) if p['fixed'] else (real, c('match_box'))
  cnt, cnt_box = np.maximum(1.0, match.sum(axis=(1, 2))).astype(dtype), np.maximum(1.0, match_box.sum(axis=(1, 2))).astype(dtype)
  y_gt = c('sum_gt')[:, :, None, None]  # one pixel per instance carrying its sum: all f_coverage_weight reads
  # fixed order: the reference sums the whole diagonal (full_model.py:922-924,947-951); an absent ground truth overlaps nothing
  masked = lambda iou, m: np.einsum('bii->b', iou) if p['fixed'] else (iou * m).sum(axis=(1, 2))
  o = {}
  o['iou_soft'] = (masked(c('iou_soft'), match) / cnt).sum() / B
  o['iou_soft_box'] = (masked(c('iou_box'), match_box) / cnt_box).sum() / B
  o['wt_cov_soft'] = ora.f_weighted_coverage(c('iou_soft'), y_gt)
  o['unwt_cov_soft'] = ora.f_unweighted_coverage(c('iou_soft'), cnt)
  o['wt_cov_hard'] = ora.f_weighted_coverage(c('iou_hard'), y_gt)
  o['unwt_cov_hard'] = ora.f_unweighted_coverage(c('iou_hard'), cnt)
  o['iou_hard'] = ((c('iou_hard') * real).sum(axis=(1, 2)) / cnt).sum() / B
  o['dice'] = ((c('dice') * real).sum(axis=(1, 2)) / cnt).sum() / B
  o['conf_loss'] = ora.f_conf_loss(s_out, match)
  o['count_acc'], o['dic'], o['dic_abs'] = ora.f_count_stats(s_out, s_gt)
  o['box_loss'] = -o['iou_soft_box']
  o['segm_loss'] = -o['wt_cov_soft'] if p['fn'] else -o['iou_soft']
  o['loss'] = o['box_loss'] + o['segm_loss'] + dtype(p['mix']) * o['conf_loss']
  import ra_ops
  return {'stats': np.array([float(o[k]) for k in ra_ops.STAT_NAMES])}


def _wsum_reference(r, x, dtype, zero_row_skips_bias=False):
  out = np.einsum('bnt,btp->bnp', x['w'].astype(dtype), x['y'].astype(dtype))
  if 'bias' in x:
    bias = x['bias'].astype(dtype)[:, :, None]
    if zero_row_skips_bias:
      bias = bias * (x['w'] != 0).any(axis=2)[:, :, None]
    out = out + bias
  return {'out': out.astype(np.float64)}


def _canvas_reference(r, x, dtype=None, lane_of_group0=False):
  """The element-wise chain ra_canvas_step_f32 replaced, float32 NumPy, every product and sum rounded on its own, in its order."""
  p = r.p
  yc = x['y'].copy()
  if 'match' in x:
    g = np.zeros_like(yc)
    for t in range(p['T']):
      wt = x['match'][:, t]
      term = g + wt[:, None] * x['y_gt'][:, t]
      g = np.where((wt != 0)[:, None], term, g).astype(np.float32)
    if 'noise' in x:
      g = g - g * x['noise']
    k = x['knob'][:, 0][:, None]
    yc = k * g + (np.float32(1.0) - k) * yc
  assert yc.dtype == np.float32
  nxt = x['prev'].copy()
  cc = (p['cc'] & 3) if lane_of_group0 else p['cc']
  nxt[:, :, cc] = np.maximum(yc, x['prev'][:, :, cc])
  return {'next': nxt}


def _pair_reference(r, x, dtype, drop_last_group=False):
  a, b = x['a'].astype(dtype), x['b'].astype(dtype)
  if drop_last_group:  # the mutant: the last 4-pixel group of every 4096-pixel chunk never read
    a, b = a.copy(), b.copy()
    for end in range(4096, a.shape[2] + 1, 4096):
      a[:, :, end - 4:end], b[:, :, end - 4:end] = 0, 0
  a4, b4 = a[:, :, :, None], b[:, :, :, None]
  ah = (a4 > 0.5).astype(dtype)
  o = {'iou_soft': ora.f_iou_pairwise(a4, b4), 'iou_hard': ora.f_iou_pairwise(ah, b4), 'dice_hard': ora.f_dice_pairwise(ah, b4),
       'sum_a': a.sum(axis=2), 'sum_b': b.sum(axis=2), 'inter': np.einsum('bnp,bmp->bnm', a, b), 'sum_a_hard': ah.sum(axis=(2, 3))}
  o['iou_soft_torch'] = orat.iou_pairwise(torch.from_numpy(a4), torch.from_numpy(b4)).numpy()  # the torch oracle's restatement: the same
  return {k: v.astype(np.float64) for k, v in o.items()}


def _box_reference(r, x, dtype, truncate_T=False, last_slice_min_lost=False):
  p = r.p
  B, T, H, W = p['B'], p['T'], p['H'], p['W']
  y = x['y_gt'].astype(dtype)
  tl, br, box = ora.get_gt_box(y, padding_ratio=dtype(BOX_PAD_RATIO), center_shift_ratio=dtype(0.0), min_padding=dtype(BOX_MIN_PAD))
  nz = (y.sum(axis=(2, 3)) > 0)[:, :, None]
  # fields 4..7: the padded rectangle before the empty-instance fix-up (an empty instance: min = H W, max = 0, size < 0)
  far = dtype(H * W) - dtype(BOX_MIN_PAD)
  params = np.concatenate([tl, br, np.where(nz, tl, far), np.where(nz, br, dtype(BOX_MIN_PAD))], axis=2)
  if last_slice_min_lost:  # the mutant: the minimum of the last of the eight slices never combined
    per = -(-(H * W // 4) // 8) * 4
    cut = y.reshape(B, T, -1).copy()
    cut[:, :, 7 * per:] = 0
    tl2 = ora.get_gt_box(cut.reshape(y.shape), padding_ratio=dtype(BOX_PAD_RATIO), center_shift_ratio=dtype(0.0), min_padding=dtype(BOX_MIN_PAD))[0]
    params[:, :, 0:2], params[:, :, 4:6] = tl2, np.where((cut.sum(axis=2) > 0)[:, :, None], tl2, far)
  o = {'params': params, 'box': box}
  # the noisy ground-truth attention (full_model.py:567-577) and the knobs (:596-625)
  tln, brn, _ = ora.get_gt_box(y, padding_ratio=x['pad'].astype(dtype)[:, :, None], center_shift_ratio=x['shift'].astype(dtype), min_padding=dtype(BOX_MIN_PAD))
  o['ctr'], o['size'] = (tln + brn) / 2, brn - tln
  thr = knob_thresholds(T, p['seed'] % 2, dtype)
  o['knob_box'], o['knob_segm'] = [(x[k].astype(dtype) <= thr[i][None, :]).astype(dtype) for i, k in enumerate(('u_box', 'u_segm'))]
  o['ctr_chain'], o['size_chain'] = knob_chain(x, H, W)
  iou = ora.f_iou_pairwise(x['map'].astype(dtype)[:, None], box)[:, 0]
  if truncate_T:  # the mutant: the unrolled rectangle loop one short of TM
    iou = iou.copy()
    iou[:, launch_choices(r)['TM'] - 1:] = 0
  o['iou'] = iou
  return {k: np.asarray(v, dtype=np.float64) for k, v in o.items()}


def knob_chain(x, H, W):
  """ctr, size of ra_knob_setup_f32 as the element-wise float32 chain it replaced takes them (TrainStep._knob_setup without the
  fused kernel; modellib.get_gt_box's order), every product and sum rounded on its own: what the kernel must give bit for bit."""
  y, one = x['y_gt'], np.float32(1.0)
  yy, xx = np.arange(H, dtype=np.float32)[None, None, :, None], np.arange(W, dtype=np.float32)[None, None, None, :]
  big, mp = np.float32(H * W), np.float32(BOX_MIN_PAD)
  tl = np.stack([(i + (one - y) * big).min(axis=(2, 3)) for i in (yy, xx)], axis=2)
  br = np.stack([(i * y).max(axis=(2, 3)) for i in (yy, xx)], axis=2)
  nz = (y.sum(axis=(2, 3), dtype=np.float64) > 0).astype(np.float32)[:, :, None]
  sz = br - tl
  padv, sh = np.maximum(x['pad'][:, :, None] * sz, mp), x['shift'] * sz
  tln = ((tl + sh) - padv) * nz
  brn = nz * ((br + sh) + padv) + (one - nz) * (np.float32(2.0) * mp)
  ctr, size = (tln + brn) / np.float32(2.0), brn - tln
  assert ctr.dtype == np.float32 and size.dtype == np.float32
  return ctr, size


_REFERENCE = {'head': _head_reference, 'stats': _stats_reference, 'wsum': _wsum_reference, 'canvas': _canvas_reference, 'pair': _pair_reference,
              'box': _box_reference}


@functools.lru_cache(maxsize=None)
def _reference_cached(family, name, dtype):
  r = ROW_OF[(family, name)]
  return _REFERENCE[family](r, inputs(r), getattr(np, dtype) if family != 'head' else dtype)


def reference(r, dtype='float64'):
  """The row's reference, computed once per process and shared: callers leave it unchanged."""
  return _reference_cached(r.family, r.name, dtype)


def mutant(r, which):
  """The reference with one plausible kernel error restated on it (float64), shaped like a kernel's result."""
  x = inputs(r)
  if which == 'chunk-tail':
    return _pair_reference(r, x, np.float64, drop_last_group=True)
  if which == 'stale-coef':  # the wave's second image adds up the first one's coef rows (its own idx)
    return dict(reference(r), ds=head_ds(x, r.p, np.float64, coef_of=lambda b: b - 4 if b >= 4 else b))
  if which == 'no-clamp':
    with np.errstate(all='ignore'):
      return _head_reference(r, x, 'float64', clamp=False)
  if which == 'other-tie':
    return dict(reference(r), ds=head_ds(x, r.p, np.float64, first_min=True))
  if which == 'tm-1':
    return _box_reference(r, x, np.float64, truncate_T=True)
  if which == 'last-slice':
    return _box_reference(r, x, np.float64, last_slice_min_lost=True)
  if which == 'group0':
    return _canvas_reference(r, x, lane_of_group0=True)
  if which == 'zero-row':
    return _wsum_reference(r, x, np.float64, zero_row_skips_bias=True)
  raise KeyError(which)


# ---- scoring: [(what, err, bar), ...]; a row passes where every err < bar

def _rel1(got, ref):
  """|got - ref| max over max(1, |ref| max); NaN or a wrong shape is inf."""
  got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
  assert got.shape == ref.shape, (got.shape, ref.shape)
  if got.size == 0:
    return 0.0
  e = np.abs(got - ref).max() / max(1.0, np.abs(ref).max())
  return float(e) if np.isfinite(e) else np.inf


def _each1(got, ref):
  """Per element: |got - ref| over max(1, |ref|), the largest."""
  got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
  e = (np.abs(got - ref) / np.maximum(1.0, np.abs(ref))).max()
  return float(e) if np.isfinite(e) else np.inf


def _absmax(got, ref):
  e = np.abs(np.asarray(got, dtype=np.float64) - np.asarray(ref, dtype=np.float64)).max()
  return float(e) if np.isfinite(e) else np.inf


def _differ(got, ref):
  got, ref = np.asarray(got), np.asarray(ref)
  assert got.shape == ref.shape, (got.shape, ref.shape)
  return int((got.astype(np.float64) != ref.astype(np.float64)).sum())


def _grad(got, ref):
  e = _per_image(got, ref, 0, True)
  return e if np.isfinite(e) else np.inf


COUNT_STATS = ('count_acc', 'dic', 'dic_abs')


def scores(r, ref, got):
  p, x, out = r.p, inputs(r), []
  if r.family == 'head':
    out.append(('pieces', _each1(got['pieces'], ref['pieces']), TOL_PIECES))
    for k in ('c1_s', 'c0_s', 'c1_b', 'c0_b', 'ds'):
      out.append((k, _grad(got[k], ref[k]), TOL_GRAD))
    for h in 'sb':
      out.append(('c1_%s where m == 0' % h, int((np.asarray(got['c1_' + h])[x['m_' + h] == 0] != 0).sum()), EXACT))
    if p['mix'] == 0:
      out.append(('ds at mix 0', int((np.asarray(got['ds']) != 0).sum()), EXACT))
  elif r.family == 'stats':
    import ra_ops
    for k, name in enumerate(ra_ops.STAT_NAMES):
      if name in COUNT_STATS:
        out.append((name, _differ(np.float32(got['stats'][k:k + 1]), np.float32(ref['stats'][k:k + 1])), EXACT))  # the float32 of the exact ratio
      else:
        out.append((name, _each1(got['stats'][k:k + 1], ref['stats'][k:k + 1]), TOL_STATS))
  elif r.family == 'wsum':
    out.append(('out', _rel1(got['out'], ref['out']), TOL_WSUM))
    zero = ~(x['w'] != 0).any(axis=2)
    bias = x['bias'] if 'bias' in x else np.zeros(zero.shape, np.float32)
    out.append(('zero-weight rows', _differ(np.asarray(got['out'])[zero], np.broadcast_to(bias[:, :, None], got['out'].shape)[zero]), EXACT))
  elif r.family == 'canvas':
    cc = p['cc']
    out.append(('canvas channel', _differ(np.asarray(got['next'])[:, :, cc], ref['next'][:, :, cc]), EXACT))
    out.append(('copied channels', _differ(np.delete(np.asarray(got['next']), cc, axis=2), np.delete(x['prev'], cc, axis=2)), EXACT))
  elif r.family == 'pair':
    for k in ('iou_soft', 'iou_hard', 'dice_hard', 'sum_a', 'sum_b', 'inter'):
      out.append((k, _rel1(got[k], ref[k]), TOL_PAIR))
    out.append(('sum_a_hard', _differ(got['sum_a_hard'], ref['sum_a_hard']), EXACT))
  elif r.family == 'box':
    out.append(('params', _each1(got['params'], ref['params']), TOL_BOX))
    out.append(('box', _differ(got['box'], ref['box']), EXACT))
    out.append(('ctr', _each1(got['ctr'], ref['ctr']), TOL_CTR))
    out.append(('size', _each1(got['size'], ref['size']), TOL_SIZE))
    if np.asarray(got['ctr']).dtype == np.float32:  # a kernel's result (the references come back as float64)
      out.append(('ctr, size: the float32 chain', _differ(got['ctr'], ref['ctr_chain']) + _differ(got['size'], ref['size_chain']), EXACT))
    out.append(('knob_box', _differ(got['knob_box'], ref['knob_box']), EXACT))
    out.append(('knob_segm', _differ(got['knob_segm'], ref['knob_segm']), EXACT))
    out.append(('iou', _rel1(got['iou'], ref['iou']), TOL_RECT))
  return out


def failures(score_list):
  return [w for w, e, bar in score_list if not e < bar]


# ---- the input conditions (tests/test_loss_train.py asserts them for every row)

def rect_corner_margin(ref):
  """The smallest distance of a padded rectangle's corner from an integer."""
  c = ref['params'][:, :, 4:8]
  return float(np.abs(c - np.round(c)).min())


def conditions(r):
  """name -> bool, each a condition the row's inputs are meant to satisfy."""
  p, x, c = r.p, inputs(r), collections.OrderedDict()
  if r.family == 'head':
    s = x['s_out'].astype(np.float64)
    gaps = np.diff(np.sort(s, axis=1), axis=1)
    if p['ties']:
      c['ties planted'] = bool((gaps == 0).sum() >= 3 and (s == 1.0).sum() >= 3)
      moved = np.abs(head_ds(x, p, np.float64) - head_ds(x, p, np.float64, first_min=True))
      c['the tie rule matters for a minimum, a maximum and the run of ones'] = bool(all(moved[b].max() > 0 for b in range(3)))
    else:
      c['scores in (0.02, 0.98), more than MARGIN apart'] = bool(s.min() > 0.02 and s.max() < 0.98 and (p['T'] == 1 or gaps.min() >= MARGIN))
    cs, cb = x['m_s'].sum(axis=(1, 2)), x['m_b'].sum(axis=(1, 2))
    c['an unmatched image'] = bool((cs == 0).any() or (cb == 0).any())
    c['a fully matched image'] = bool((cs == p['T']).any())
    c['m_s and m_b differ'] = not np.array_equal(x['m_s'], x['m_b'])
    c['partial permutations'] = bool(all(m.sum(axis=1).max() <= 1 and m.sum(axis=2).max() <= 1 for m in (x['m_s'], x['m_b'])))
    c['iou in (0, 1)'] = bool(min(x['iou_s'].min(), x['iou_b'].min()) > 0 and max(x['iou_s'].max(), x['iou_b'].max()) < 1)
    eps_share = 1e-5 * p['HW'] / (x['sa_s'][:, :, None] + x['sb_s'][:, None, :] - x['inter_s'] + 1e-5 * p['HW'])
    c['the 1e-5 HW term from negligible to dominant'] = bool(p['HW'] < 1000 or p['B'] * p['T'] < 10 or (eps_share.max() > 0.5 and eps_share.min() < 1e-3))
  elif r.family == 'stats':
    s = x['s_out'].astype(np.float64)
    d = np.abs(s - 0.5)
    c['one score exactly 0.5, the others MARGIN away'] = bool((d == 0).sum() == 1 and (d[d > 0].min() if (d > 0).any() else 1) >= MARGIN)
    if p['B'] >= 2:
      c['an image with no ground truth'] = bool((x['s_gt'][0] == 0).all() and (x['sum_gt'][0] == 0).all())
      c['an image with no match'] = bool((x['match_real'].sum(axis=(1, 2)) == 0).any())
    if p['B'] >= 3:
      c['an image with ground truth and no match'] = bool(x['s_gt'][1].sum() > 0 and x['match_real'][1].sum() == 0)
    c['match_box != match_real'] = bool(p['T'] == 1 or not np.array_equal(x['match_box'], x['match_real']))
    c['an absent ground truth overlaps nothing'] = bool(all((x[k] * (1 - x['s_gt'][:, None, :]) == 0).all() for k in ('iou_soft', 'iou_hard', 'dice', 'iou_box')))
  elif r.family == 'wsum':
    zero = ~(x['w'] != 0).any(axis=2)
    c['a row of zeros, and only one'] = bool(zero.sum() == 1)
    c['zeros among the other weights'] = bool(p['T'] == 1 or ((x['w'] == 0).sum() > p['T']))
  elif r.family == 'canvas':
    if p['form'] != 'nomatch':
      c['a one-hot and an all-zero match row'] = bool(sorted(x['match'][0]) == [0] * (p['T'] - 1) + [1] and (x['match'][1] == 0).all())
      c['knobs 0, 1 and a fraction'] = bool(x['knob'][0, 0] == 0 and x['knob'][1, 0] == 1 and 0 < x['knob'][2, 0] < 1)
  elif r.family == 'pair':
    d = np.abs(x['a'].astype(np.float64) - 0.5)
    c['a handful of a exactly 0.5, the others MARGIN away'] = bool(1 <= (d == 0).sum() <= 5 and d[d > 0].min() >= MARGIN)
    c['an empty a plane and an empty b plane'] = bool((x['a'][0, -1] == 0).all() and (x['b'][0, 0] == 0).all())
  elif r.family == 'box':
    ref = reference(r)
    c['corners MARGIN from an integer'] = rect_corner_margin(ref) >= MARGIN
    n = p['B'] * p['T']
    sums = x['y_gt'].reshape(n, -1).sum(axis=1)
    if n >= 4:
      c['an empty, a one-pixel, a soft instance'] = bool(sums[1] == 0 and sums[0] == 1 and set(np.unique(x['y_gt'].reshape(n, -1)[3])) == {0.0, 0.5})
      c['a rectangle entirely outside'] = bool(ref['iou'].reshape(-1)[1] == 0 and ref['box'].reshape(n, -1)[1].sum() == 0)
    rect = ref['params'][:, :, 4:8].reshape(n, 4)
    c['padded rectangles reach outside on each side'] = bool(n < 5 or ((rect[:, 0] < 0).any() and (rect[:, 1] < 0).any() and (rect[:, 2] > p['H'] - 1).any() and
                                                                       (rect[:, 3] > p['W'] - 1).any()))
    thr = knob_thresholds(p['T'], p['seed'] % 2)
    c['u MARGIN from its threshold'] = bool(min(np.abs(x[k].astype(np.float64) - thr[i][None]).min() for i, k in enumerate(('u_box', 'u_segm'))) >= MARGIN)
  return c


# ---- the kernels through the C ABI (needs an MI355X)

def Guarded(shape, dev):
  from test_conv_forms_gpu import Guarded as G
  return G(shape, dev)


def SENTINEL():
  import test_conv_forms_gpu
  return test_conv_forms_gpu.SENTINEL


def to_dev(x, dev):
  return {k: torch.from_numpy(v).to(dev) for k, v in x.items()}


def bits_of(bufs):
  """The whole buffers (guards included) of a dict of Guarded, as bytes."""
  torch.cuda.synchronize()
  return b''.join(bufs[k].buf.view(torch.int32).cpu().numpy().tobytes() for k in sorted(bufs))


def _results(bufs, what):
  return {k: v.result('%s %s' % (what, k)) for k, v in bufs.items()}


def head_buffers(r, dev):
  B, T = r.p['B'], r.p['T']
  # pieces: six floats, what recattend.h documents — the guard behind them is the check
  return {'pieces': Guarded((6,), dev), 'c1_s': Guarded((B, T, T), dev), 'c0_s': Guarded((B, T), dev), 'c1_b': Guarded((B, T, T), dev),
          'c0_b': Guarded((B, T), dev), 'ds': Guarded((B, T), dev)}


def head_call(r, xd, bufs):
  """(rc forward, rc backward)."""
  import ra_native as rn
  p, v = r.p, lambda k: rn.ptr(bufs[k].view)
  x = lambda k: rn.ptr(xd[k])
  rc1 = rn.lib().ra_loss_head_f32(x('iou_s'), x('iou_b'), x('m_s'), x('m_b'), x('s_out'), p['B'], p['T'], p['mix'], v('pieces'), rn.stream_ptr())
  rc2 = rn.lib().ra_loss_head_bwd_f32(x('g') if 'g' in xd else None, x('m_s'), x('m_b'), x('s_out'), x('inter_s'), x('sa_s'), x('sb_s'), x('inter_b'), x('sa_b'),
                                      x('sb_b'), p['B'], p['T'], p['HW'], p['mix'], v('c1_s'), v('c0_s'), v('c1_b'), v('c0_b'), v('ds'), rn.stream_ptr())
  return rc1, rc2


def stats_buffers(r, dev):
  return {'stats': Guarded((15,), dev), 'ws': Guarded((12 * r.p['B'],), dev)}


def stats_call(r, xd, bufs, T=None):
  import ra_native as rn
  p, x = r.p, lambda k: rn.ptr(xd[k])
  assert rn.lib().ra_loss_stats_workspace_floats(p['B']) == 12 * p['B']
  return rn.lib().ra_loss_stats_f32(x('iou_soft'), x('iou_hard'), x('dice'), x('match_real'), x('iou_box'), x('match_box'), x('s_out'), x('s_gt'), x('sum_gt'),
                                    p['B'], p['T'] if T is None else T, p['fixed'], p['fn'], p['mix'], rn.ptr(bufs['ws'].view), 12 * p['B'],
                                    rn.ptr(bufs['stats'].view), rn.stream_ptr())


WSUM_FORMS = ('dense', 'tmajor', 'tmajor-gap')  # out [B,N,HW]; [N,B,HW] through strides; the same with 8 floats between the planes' rows
WSUM_GAP = 8


def wsum_strides(r, form):
  """(o_img, o_row, floats of the buffer)."""
  B, N, HW = r.p['B'], r.p['N'], r.p['HW']
  if form == 'dense':
    return N * HW, HW, B * N * HW
  o_row = B * HW + (WSUM_GAP if form == 'tmajor-gap' else 0)
  return HW, o_row, N * o_row


def wsum_buffers(r, dev, form):
  o_img, o_row, n = wsum_strides(r, form)
  g = Guarded((n,), dev)
  if form == 'tmajor-gap':
    g.view.view(r.p['N'], o_row)[:, r.p['B'] * r.p['HW']:].view(torch.int32).fill_(SENTINEL())
  return {'out': g}


def wsum_call(r, xd, bufs, form, strides=None):
  import ra_native as rn
  p = r.p
  o_img, o_row, _ = wsum_strides(r, form)
  if strides is not None:
    o_img, o_row = strides
  args = (rn.ptr(xd['w']), rn.ptr(xd['bias']) if 'bias' in xd else None, rn.ptr(xd['y']), p['B'], p['N'], p['T'], p['HW'], rn.ptr(bufs['out'].view))
  if form == 'dense':
    return rn.lib().ra_weighted_sum_multi_f32(*(args + (rn.stream_ptr(),)))
  return rn.lib().ra_weighted_sum_multi_strided_f32(*(args + (o_img, o_row, rn.stream_ptr())))


def wsum_results(r, bufs, form, what):
  B, N, HW = r.p['B'], r.p['N'], r.p['HW']
  g = bufs['out']
  if form == 'dense':
    return {'out': g.result(what).reshape(B, N, HW)}
  o_row = wsum_strides(r, form)[1]
  if form == 'tmajor-gap':  # the floats between the planes' rows keep their sentinel; then they are checked, and result() looks at the rest
    torch.cuda.synchronize()
    gaps = g.view.view(N, o_row)[:, B * HW:]
    assert (gaps.view(torch.int32).cpu().numpy() == SENTINEL()).all(), '%s: wrote between the rows of its planes' % what
    gaps.fill_(0.0)
  y = g.result(what).reshape(N, o_row)[:, :B * HW].reshape(N, B, HW)
  if form == 'tmajor-gap':
    gaps.view(torch.int32).fill_(SENTINEL())  # as before, for a relaunch into the same buffer
  return {'out': np.ascontiguousarray(y.transpose(1, 0, 2))}


def canvas_buffers(r, dev):
  return {'next': Guarded((r.p['B'], r.p['HW'], r.p['C']), dev)}


def canvas_call(r, xd, bufs):
  import ra_native as rn
  p, o = r.p, lambda k: rn.ptr(xd[k]) if k in xd else None
  return rn.lib().ra_canvas_step_f32(rn.ptr(xd['prev']), p['C'], p['cc'], p['B'], p['HW'], rn.ptr(xd['y']), o('match'), o('y_gt'), p['T'], o('noise'), o('knob'),
                                     p['knob_stride'], rn.ptr(bufs['next'].view), rn.stream_ptr())


PAIR_OUT = ('iou_soft', 'iou_hard', 'dice_hard', 'sum_a', 'sum_b', 'inter', 'sum_a_hard')


def pair_buffers(r, dev):
  import ra_native as rn
  B, N, M = r.p['B'], r.p['N'], r.p['M']
  shape = {'sum_a': (B, N), 'sum_b': (B, M), 'sum_a_hard': (B, N)}
  bufs = {k: Guarded(shape.get(k, (B, N, M)), dev) for k in PAIR_OUT}
  bufs['ws'] = Guarded((rn.lib().ra_pair_stats_workspace_floats(B, r.p['HW']),), dev)
  return bufs


def pair_call(r, xd, bufs, tmajor=False, dims=None, strides=None):
  """tmajor: a read in place from its [N,B,HW] copy xd['a_t'] through strides.  dims = (N, M, HW) other than the row's (a refused call)."""
  import ra_native as rn
  p = r.p
  N, M, HW = dims or (p['N'], p['M'], p['HW'])
  outs = tuple(rn.ptr(bufs[k].view) for k in PAIR_OUT)
  tail = (rn.ptr(xd['b']), p['B'], N, M, HW, rn.ptr(bufs['ws'].view), bufs['ws'].n) + outs + (rn.stream_ptr(),)
  if not tmajor:
    return rn.lib().ra_pair_stats_f32(*((rn.ptr(xd['a']),) + tail))
  a_img, a_row = strides or (HW, p['B'] * HW)
  return rn.lib().ra_pair_stats_strided_f32(*((rn.ptr(xd['a_t']), a_img, a_row) + tail))


def pair_results(bufs, what):
  bufs['ws'].result(what + ' workspace')  # the chunk records and the totals: every float written, none beyond
  return {k: bufs[k].result('%s %s' % (what, k)) for k in PAIR_OUT}


def box_buffers(r, dev):
  import ra_native as rn
  B, T, H, W = r.p['B'], r.p['T'], r.p['H'], r.p['W']
  assert rn.lib().ra_gt_box_workspace_floats(B, T) == B * T * 40 and rn.lib().ra_box_iou_rects_workspace_floats(B) == B * 64 * 33
  return {'params': Guarded((B, T, 8), dev), 'box': Guarded((B, T, H, W), dev), 'gt_ws': Guarded((B * T * 40,), dev), 'ctr': Guarded((B, T, 2), dev),
          'size': Guarded((B, T, 2), dev), 'knob_box': Guarded((B, T), dev), 'knob_segm': Guarded((B, T), dev), 'iou': Guarded((B, T), dev),
          'rect_ws': torch.zeros(B * 64 * 33, dtype=torch.float32, device=dev)}


BOX_OUT = ('params', 'box', 'ctr', 'size', 'knob_box', 'knob_segm', 'iou')


def box_call(r, xd, bufs):
  """(rc of ra_gt_box_f32, ra_knob_setup_f32, ra_box_iou_rects_f32): the three in the training step's order, the second on the
  first one's workspace, the third on the first one's params."""
  import ra_native as rn
  p, v, x = r.p, lambda k: rn.ptr(bufs[k].view), lambda k: rn.ptr(xd[k])
  B, T, H, W = p['B'], p['T'], p['H'], p['W']
  rc1 = rn.lib().ra_gt_box_f32(x('y_gt'), B, T, H, W, BOX_PAD_RATIO, BOX_MIN_PAD, v('gt_ws'), B * T * 40, v('params'), v('box'), rn.stream_ptr())
  rc2 = rn.lib().ra_knob_setup_f32(v('gt_ws'), B, T, x('pad'), x('shift'), x('u_box'), x('u_segm'), x('sched'), BOX_MIN_PAD, p['seed'] % 2, v('ctr'), v('size'),
                                   v('knob_box'), v('knob_segm'), rn.stream_ptr())
  rc3 = rn.lib().ra_box_iou_rects_f32(x('map'), v('params'), B, T, H, W, rn.ptr(bufs['rect_ws']), bufs['rect_ws'].numel(), v('iou'), rn.stream_ptr())
  return rc1, rc2, rc3


def launch(r, x, dev, bufs=None, form=None):
  """The row's kernels on inputs x into fresh guarded buffers (or bufs) -> (bufs, results shaped like reference()'s).
  form: wsum's output layout (WSUM_FORMS), pair's 'tmajor'."""
  import ra_native as rn
  xd, what = to_dev(x, dev), '%s %s' % (r.family, r.name)
  if r.family == 'head':
    bufs = bufs or head_buffers(r, dev)
    for rc, name in zip(head_call(r, xd, bufs), ('ra_loss_head_f32', 'ra_loss_head_bwd_f32')):
      rn.check(rc, name)
    return bufs, _results(bufs, what)
  if r.family == 'stats':
    bufs = bufs or stats_buffers(r, dev)
    rn.check(stats_call(r, xd, bufs), 'ra_loss_stats_f32')
    bufs['ws'].result(what + ' workspace')  # every float of it written, none beyond
    return bufs, {'stats': bufs['stats'].result(what)}
  if r.family == 'wsum':
    form = form or 'dense'
    bufs = bufs or wsum_buffers(r, dev, form)
    rn.check(wsum_call(r, xd, bufs, form), 'ra_weighted_sum_multi_f32')
    return bufs, wsum_results(r, bufs, form, '%s %s' % (what, form))
  if r.family == 'canvas':
    bufs = bufs or canvas_buffers(r, dev)
    rn.check(canvas_call(r, xd, bufs), 'ra_canvas_step_f32')
    return bufs, _results(bufs, what)
  if r.family == 'pair':
    bufs = bufs or pair_buffers(r, dev)
    if form == 'tmajor':
      xd['a_t'] = xd['a'].transpose(0, 1).contiguous()
    rn.check(pair_call(r, xd, bufs, tmajor=form == 'tmajor'), 'ra_pair_stats_f32')
    return bufs, pair_results(bufs, what)
  if r.family == 'box':
    bufs = bufs or box_buffers(r, dev)
    for rc, name in zip(box_call(r, xd, bufs), ('ra_gt_box_f32', 'ra_knob_setup_f32', 'ra_box_iou_rects_f32')):
      rn.check(rc, name)
    bufs['gt_ws'].result(what + ' workspace')  # 8 slices of 5 floats per instance, empty slices included
    return bufs, {k: bufs[k].result('%s %s' % (what, k)) for k in BOX_OUT}
  raise KeyError(r.family)


def guarded_only(bufs):
  return {k: v for k, v in bufs.items() if hasattr(v, 'buf')}


def worst_by_quantity(score_lists):
  out = collections.OrderedDict()
  for w, e, bar in score_lists:
    out[w] = (max(e, out[w][0]) if w in out else e, bar)
  return [(w, e, bar) for w, (e, bar) in out.items()]


def main():
  import argparse
  ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
  ap.add_argument('--measure', action='store_true', help='the float32 CPU run of the reference against the float64 one (host only)')
  args = ap.parse_args()
  if args.measure:
    for family, rows in ROWS.items():
      worst = {}
      for r in rows:
        for w, e, bar in scores(r, reference(r), reference(r, 'float32')):
          if w not in worst or e > worst[w][0]:
            worst[w] = (e, bar, r.name)
      for w, (e, bar, name) in worst.items():
        print('%-7s %-22s float32 CPU run %.3e at %-26s bar %g (%.1f times inside)' % (family, w, e, name, bar, bar / e if e else np.inf), flush=True)
    return
  if not torch.cuda.is_available():
    raise SystemExit('loss_train_cases: needs an MI355X')
  dev = torch.device('cuda')
  for family, rows in ROWS.items():
    for r in rows:
      sc = scores(r, reference(r), launch(r, inputs(r), dev)[1])
      print('%-6s %-26s (%s) worst %.3f of its bar' % (family, r.name, ' '.join('%s %s' % kv for kv in r.p.items() if kv[0] != 'seed'),
                                                       max(e / bar for _, e, bar in sc)))
      for w, e, bar in sc:
        print(('  %-22s %d differ  (exact)' % (w, e)) if bar == EXACT else ('  %-22s %.3e  bar %g' % (w, e, bar)), flush=True)


if __name__ == '__main__':
  main()
