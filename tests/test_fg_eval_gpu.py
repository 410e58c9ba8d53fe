"""Evaluating the pre-stage on the MI355X: the statistics kernel (ra_fg_stats_f32) and fg_model.Model.statistics against the
float64 oracle of fg_model.py:196-246, the fused threshold sweep (ra_fg_sweep_counts_f32) against the float64 oracle of
fg_model_eval.py:134-178 by the band rule of the stage tests and against the plane kernels on the device, and the command line
end to end.

Bars.  Statistics: the integer-valued sums are equal; the float sums and the six statistics are within 2e-5 relative (the
project's mask tolerance; floor 1e-7 absolute) of the oracle fed the same float32 logits — the design bounds the error at
64 * 2^-24 = 4e-6 plus a few ulp of expf / logf.  Sweep: with v64 the oracle's filtered value and d = 1e-5, every counter lies
between its value over v64 > thr + d and over v64 > thr - d, and the pixels inside that band are at most 0.1 % of the image
per threshold (a condition on the inputs, asserted)."""
import functools
import os

import numpy as np
import pytest
import torch

import analysis
import fg_eval_oracle as feo
import fg_model
import fg_model_eval
import fg_oracle as fo
import ra_native as rn
import ra_ops as ops
from utils import png

pytestmark = pytest.mark.gpu
TOL = 2e-5     # relative, the float sums and the statistics
FLOOR = 1e-7   # absolute
DELTA = 1e-5   # the band of the sweep
BAND_SHARE = 1e-3
INTEGER_SUMS = ('sum_gt', 'mask', 'inter_hard', 'sum_hard', 'ori_correct')


def _dev(a, dtype=np.float32):
  return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


# ------------------------------------------------------------------------------------------------------------ statistics kernel
STAT_SHAPES = [(2, 9, 11, 1, 0), (2, 9, 11, 1, 8), (3, 64, 96, 9, 8), (1, 16, 16, 16, 0)]


def _one_hot(idx, n):
  return np.eye(n, dtype=np.float32)[idx]


@functools.lru_cache(maxsize=None)
def _stat_case(shape, kind='random'):
  B, H, W, nsc, no = shape
  rng = np.random.RandomState(sum(shape) + 7 * len(kind))
  if kind == 'ties':  # small integers: equal class maxima, logits of exactly 0, equal orientation maxima on both sides
    lg = rng.randint(-2, 3, (B, H, W, nsc + no)).astype(np.float32)
  else:
    lg = (rng.randn(B, H, W, nsc + no) * 2.5).astype(np.float32)
  if nsc == 1:
    g = (rng.rand(B, H, W, 1) > 0.6).astype(np.float32)
  else:
    g = _one_hot(rng.randint(0, nsc, (B, H, W)), nsc)
  if kind == 'background':
    g = np.zeros_like(g)
    if nsc > 1:
      g[..., 0] = 1
  d = None
  if no:
    d = (rng.randint(0, 2, (B, H, W, no)).astype(np.float32) if kind == 'ties' else _one_hot(rng.randint(0, no, (B, H, W)), no))
  return lg, g, d, feo.sums(lg, g, d, nsc, no)


def _check_sums(got, ref, what):
  for k in feo.SUM_NAMES:
    err = abs(got[k] - ref[k])
    print('%s %-12s got %.10g ref %.10g  |err| %.3g (rel %.3g)' % (what, k, got[k], ref[k], err, err / max(abs(ref[k]), 1e-300)))
  for k in feo.SUM_NAMES:
    if k in INTEGER_SUMS:
      assert got[k] == ref[k], (what, k, got[k], ref[k])
    else:
      assert abs(got[k] - ref[k]) <= max(TOL * abs(ref[k]), FLOOR), (what, k, got[k], ref[k])


def _check_statistics(got, ref, what):
  assert set(got) == set(ref)
  for k in sorted(ref):
    if np.isnan(ref[k]):
      assert np.isnan(got[k]), (what, k, got[k])
      continue
    err = abs(got[k] - ref[k])
    print('%s %-16s got %.10g ref %.10g  |err| %.3g' % (what, k, got[k], ref[k], err))
    assert err <= max(TOL * abs(ref[k]), FLOOR), (what, k, got[k], ref[k])


@pytest.mark.parametrize('shape', STAT_SHAPES, ids=lambda s: 'x'.join(str(v) for v in s))
def test_statistics_kernel_matches_float64_oracle(cuda, shape):
  B, H, W, nsc, no = shape
  lg, g, d, ref = _stat_case(shape)
  got = ops.fg_statistics(_dev(lg), _dev(g), None if d is None else _dev(d), nsc, no)
  _check_sums(got, ref, str(shape))
  for fn in ('iou', 'bce'):
    _check_statistics(feo.statistics_of(got, float(B * H * W), fn, bool(no)), feo.statistics_of(ref, float(B * H * W), fn, bool(no)),
                      '%s %s' % (shape, fn))


@pytest.mark.parametrize('shape', [(2, 9, 11, 1, 8), (3, 64, 96, 9, 8), (1, 16, 16, 16, 0)], ids=lambda s: 'x'.join(str(v) for v in s))
def test_statistics_kernel_constructed_ties(cuda, shape):
  B, H, W, nsc, no = shape
  lg, g, d, ref = _stat_case(shape, 'ties')
  if nsc > 1:  # the case has what it is for: pixels with several equal class maxima
    assert ((lg[..., :nsc] == lg[..., :nsc].max(axis=-1, keepdims=True)).sum(axis=-1) > 1).mean() > 0.1
  else:
    assert (lg[..., 0] == 0).any()
  got = ops.fg_statistics(_dev(lg), _dev(g), None if d is None else _dev(d), nsc, no)
  _check_sums(got, ref, 'ties %s' % (shape,))


@pytest.mark.parametrize('shape', [(2, 9, 11, 1, 8), (3, 64, 96, 9, 8)], ids=lambda s: 'x'.join(str(v) for v in s))
def test_statistics_kernel_all_background(cuda, shape):
  B, H, W, nsc, no = shape
  lg, g, d, ref = _stat_case(shape, 'background')
  got = ops.fg_statistics(_dev(lg), _dev(g), _dev(d), nsc, no)
  _check_sums(got, ref, 'background %s' % (shape,))
  assert got['mask'] == 0 and got['ori_ce'] == 0 and got['sum_gt'] == 0
  st = feo.statistics_of(got, float(B * H * W), 'bce', True)
  assert np.isnan(st['orientation_acc']) and st['iou_soft'] == 0


def test_statistics_kernel_is_run_to_run_identical(cuda):
  shape = (3, 64, 96, 9, 8)
  lg, g, d, _ = _stat_case(shape)
  a, b, c = _dev(lg), _dev(g), _dev(d)
  runs = [ops.fg_statistics(a, b, c, 9, 8) for _ in range(3)]
  assert runs[0] == runs[1] == runs[2]  # float64 values, bit for bit


# ------------------------------------------------------------------------------------------------------------ Model.statistics
NET_TOL = 2e-5  # what test_fg_model_gpu.py allows y_out / d_out (absolute)


def _ratio_bound(num, den, dnum, dden):
  """|d(num / den)| when |d num| <= dnum and |d den| <= dden < den"""
  return (dnum + abs(num / den) * dden) / (den - dden) if den > dden else np.inf


def _propagated(ref, g, d_gt, nsc, no, npix, seg):
  """Bounds on the error of the statistics when every value of y_out / d_out is off by at most NET_TOL: each soft term moves
  by NET_TOL, a log(y + eps) by NET_TOL / (y + eps - NET_TOL), and a hard decision can only change where the oracle's own
  decision is closer than NET_TOL to the threshold (one class) or the two largest values closer than 2 NET_TOL."""
  t, e = NET_TOL, feo.EPS
  y = ref['y_out']
  g = np.asarray(g, np.float64).reshape(y.shape)
  if nsc == 1:
    ys, gs, mask = y, g, g
    unsure = (np.abs(y - 0.5) <= t).astype(np.float64)
    d_ce = (g * t / (y + e - t) + (1 - g) * t / (1 - y + e - t)).sum()
  else:
    ys, gs, mask = y[..., 1:], g[..., 1:], g[..., 1:].max(axis=-1, keepdims=True)
    top = np.sort(y, axis=-1)
    unsure = np.repeat((top[..., -1:] - top[..., -2:-1] <= 2 * t).astype(np.float64), nsc - 1, axis=-1)
    d_ce = (g * t / (y + e - t)).sum()
  s = feo.sums(ref['logits'], g, d_gt, nsc, no)
  b = {}
  d_is, d_ss, d_ih, d_sh = t * gs.sum(), t * ys.size, (unsure * gs).sum(), unsure.sum()
  b['iou_soft'] = _ratio_bound(s['inter_soft'], s['sum_soft'] + s['sum_gt'] - s['inter_soft'] + e, d_is, d_ss + d_is)
  b['iou_hard'] = _ratio_bound(s['inter_hard'], s['sum_hard'] + s['sum_gt'] - s['inter_hard'] + e, d_ih, d_sh + d_ih)
  b['foreground_loss'] = b['iou_soft'] if seg == 'iou' else d_ce / npix
  b['loss'] = b['foreground_loss']
  if no:
    dd, dg = ref['d_out'], np.asarray(d_gt, np.float64)
    dtop = np.sort(dd, axis=-1)
    flips = ((dtop[..., -1:] - dtop[..., -2:-1] <= 2 * t) * mask).sum()
    b['orientation_ce'] = (dg * mask * t / (dd + e - t)).sum() / s['mask']
    b['orientation_acc'] = flips / s['mask']
    b['loss'] = b['foreground_loss'] + b['orientation_ce']
  return s, b


@pytest.mark.parametrize('nsc,orientation,seg', [(1, True, 'bce'), (3, True, 'iou'), (1, False, 'iou'), (3, False, 'bce')])
def test_model_statistics(cuda, nsc, orientation, seg):
  opt = dict(fo.reduced_opt(nsc, orientation), segm_loss_fn=seg)
  no = 8 if orientation else 0
  P = fo.random_weights(opt, 40 + nsc)
  rng = np.random.RandomState(50 + nsc)
  B, H, W = 2, 32, 48
  x = rng.rand(B, H, W, 3).astype(np.float32)
  g = (rng.rand(B, H, W) > 0.5).astype(np.float32) if nsc == 1 else _one_hot(rng.randint(0, nsc, (B, H, W)), nsc)
  d = _one_hot(rng.randint(0, 8, (B, H, W)), 8) if orientation else None
  ref = fo.forward(opt, P, x)
  s, bound = _propagated(ref, g, d, nsc, no, float(B * H * W), seg)
  want = feo.statistics_of(s, float(B * H * W), seg, orientation)
  m = fg_model.get_model(opt).load_weights(P)
  got = m.statistics(_dev(x), _dev(g), None if d is None else _dev(d))
  assert set(got) == set(want)
  for k in sorted(want):
    err = abs(got[k] - want[k])
    print('nsc %d ori %d %s %-16s got %.8g ref %.8g |err| %.3g (propagated bound %.3g)' % (nsc, orientation, seg, k, got[k], want[k], err,
                                                                                           bound[k]))
    assert err <= bound[k] + FLOOR, (k, got[k], want[k], bound[k])
  # no foreground in the ground truth: the reference's 0 / 0
  g0 = np.zeros_like(g)
  if nsc > 1:
    g0[..., 0] = 1
  got0 = m.statistics(_dev(x), _dev(g0), None if d is None else _dev(d))
  assert got0['iou_soft'] == 0 and got0['iou_hard'] == 0
  if orientation:
    assert np.isnan(got0['orientation_acc']) and np.isnan(got0['loss'])
  # what stays refused, and the argument checks
  with pytest.raises(rn.RecAttendError, match='eval only'):
    m.run(['loss'], {'x': x, 'phase_train': False})
  with pytest.raises(rn.RecAttendError):
    m.statistics(_dev(x), _dev(g[:, :-1]), None if d is None else _dev(d))
  if not orientation:
    with pytest.raises(rn.RecAttendError, match='orientation'):
      m.statistics(_dev(x), _dev(g), _dev(_one_hot(rng.randint(0, 8, (B, H, W)), 8)))


# ------------------------------------------------------------------------------------------------------------------ sweep kernel
SWEEP_SHAPES = [(2, 24, 40, 61, 103), (1, 32, 64, 128, 256), (1, 16, 16, 16, 16), (1, 8, 12, 5, 7), (3, 4, 4, 2, 3), (3, 1, 1, 1, 4)]


def _thresholds(K, seed=0):
  t = np.array([0.3]) if K == 1 else (np.arange(10) * 0.1 if K == 10 else np.linspace(0.0, 0.9, K))
  return [float(v) for v in np.random.RandomState(seed).permutation(t)]  # unsorted


@functools.lru_cache(maxsize=None)
def _sweep_case(shape):
  N, Hs, Ws, H, W = shape
  rng = np.random.RandomState(11 + sum(shape))
  src = feo.smooth_map(rng, N, Hs, Ws)
  return src, feo.upsample(src, H, W), feo.disc_labels(rng, N, H, W)


def _band(v64, gt, thr):
  lo, hi = feo.sweep_counts(v64, gt, thr, +DELTA), feo.sweep_counts(v64, gt, thr, -DELTA)
  inside = np.stack([((v64 > t - DELTA) & ~(v64 > t + DELTA)).sum(axis=(1, 2)) for t in thr], axis=1)
  share = inside / float(v64.shape[1] * v64.shape[2])
  print('pixels inside the band per image and threshold: at most %d (%.4f %% of the image)' % (inside.max(), 100 * share.max()))
  assert share.max() <= BAND_SHARE  # a condition on the inputs
  return lo, hi


def _assert_in_band(got, lo, hi, what):
  for name, g, l, h in (('count_a', got[0], lo[0], hi[0]), ('sum_ab', got[1], lo[1], hi[1])):
    assert g.shape == l.shape and (l <= g).all() and (g <= h).all(), (what, name, g, l, h)
  assert (got[2] == lo[2]).all(), (what, 'sum_b', got[2], lo[2])


def _chain_counts(src, gt, thr, H, W):
  """What the ops of the parent commit offer: the plane kernels, then torch per threshold."""
  v = ops.bilateral5(ops.resize_linear(src, H, W))
  g = gt.to(torch.int64)
  a = [(v > t) for t in thr]
  return (torch.stack([m.sum(dim=(1, 2)) for m in a], 1).cpu().numpy(), torch.stack([(m * g).sum(dim=(1, 2)) for m in a], 1).cpu().numpy(),
          g.sum(dim=(1, 2)).cpu().numpy())


@pytest.mark.parametrize('shape', SWEEP_SHAPES, ids=lambda s: '%dx%dx%d-%dx%d' % s)
def test_sweep_matches_float64_oracle_and_the_plane_kernels(cuda, shape):
  N, Hs, Ws, H, W = shape
  src, v64, gt = _sweep_case(shape)
  thr = _thresholds(10, seed=sum(shape))
  lo, hi = _band(v64, gt, thr)
  c = ops.fg_sweep_counts(_dev(src), _dev(gt, np.uint8), thr)
  assert c['pixels'] == H * W and c['count_a'].dtype == np.int64
  got = (c['count_a'], c['sum_ab'], c['sum_b'])
  _assert_in_band(got, lo, hi, 'fused')
  chain = _chain_counts(_dev(src), _dev(gt, np.uint8), thr, H, W)
  _assert_in_band(chain, lo, hi, 'plane kernels')
  print('fused == plane kernels + torch: count_a %s, sum_ab %s' % ((got[0] == chain[0]).all(), (got[1] == chain[1]).all()))


@pytest.mark.parametrize('K', [1, 16])
@pytest.mark.parametrize('labels', ['discs', 'zeros', 'ones'])
def test_sweep_threshold_counts_and_label_kinds(cuda, K, labels):
  shape = SWEEP_SHAPES[0]
  N, Hs, Ws, H, W = shape
  src, v64, gt = _sweep_case(shape)
  gt = {'discs': gt, 'zeros': np.zeros_like(gt), 'ones': np.ones_like(gt)}[labels]
  if labels == 'discs':
    assert (gt >= 2).any()  # overlapping instances
  thr = _thresholds(K, seed=K)
  lo, hi = _band(v64, gt, thr)
  c = ops.fg_sweep_counts(_dev(src), _dev(gt, np.uint8), thr)
  _assert_in_band((c['count_a'], c['sum_ab'], c['sum_b']), lo, hi, '%s K=%d' % (labels, K))
  assert c['count_a'].shape == (N, K)
  if labels == 'zeros':
    assert not c['sum_ab'].any() and not c['sum_b'].any()
  if labels == 'ones':
    assert (c['sum_ab'] == c['count_a']).all() and (c['sum_b'] == H * W).all()
  raw = ops.fg_sweep_counts_device(_dev(src), _dev(gt, np.uint8), thr).cpu().numpy()
  assert not raw[:, K:16].any() and not raw[:, 16 + K:32].any()  # the slots of unused thresholds
  again = ops.fg_sweep_counts_device(_dev(src), _dev(gt, np.uint8), thr).cpu().numpy()
  assert (raw == again).all()


def test_sweep_on_a_binary_block_map(cuda):
  N, Hs, Ws, H, W = 2, 24, 40, 61, 103
  rng = np.random.RandomState(5)
  src = np.kron((rng.rand(N, Hs // 8, Ws // 8) > 0.5), np.ones((8, 8))).astype(np.float32)
  gt = feo.disc_labels(rng, N, H, W)
  thr = [float(t) for t in np.arange(10) * 0.1]
  c = ops.fg_sweep_counts(_dev(src), _dev(gt, np.uint8), thr)
  assert (c['sum_b'] == gt.astype(np.int64).sum(axis=(1, 2))).all()
  assert (np.diff(c['count_a'], axis=1) <= 0).all() and (np.diff(c['sum_ab'], axis=1) <= 0).all()  # monotone in the threshold
  assert (c['count_a'][:, 0] > 0).all() and (c['count_a'] <= H * W).all() and (c['sum_ab'] <= c['sum_b'][:, None]).all()
  # the analyzers take binary device tensors as well as counters
  v = ops.bilateral5(ops.resize_linear(_dev(src), H, W))
  for k in (0, 5):
    res = {'y_out': (v > thr[k]).to(torch.float32), 'y_gt': _dev(gt)}
    for cls in (analysis.ForegroundIOUAnalyzer, analysis.BackgroundIOUAnalyzer):
      a, b = cls(index=k), cls()
      a.stage({'fg_counts': c}), b.stage(res)
      assert (a.inter, a.union) == (b.inter, b.union)


# ------------------------------------------------------------------------------------------------------------------ command line
E2E_DELTA = NET_TOL + DELTA  # the net's y_out is within NET_TOL of the oracle's, and resize / filter are averages of it


def test_command_line_end_to_end(cuda, tmp_path, capsys):
  import yaml
  opt = dict(fo.reduced_opt(1, True), segm_loss_fn='bce')
  P = fo.random_weights(opt, 61)
  res = str(tmp_path / 'results')
  os.makedirs(os.path.join(res, 'fg'))
  with open(os.path.join(res, 'fg', 'model_opt.yaml'), 'w') as f:
    yaml.safe_dump(opt, f)
  np.savez(os.path.join(res, 'fg', 'weights.npz'), step=np.float32(1), **P)
  rng = np.random.RandomState(62)
  N, h, w, H, W = 3, 32, 48, 61, 103
  x = rng.rand(N, h, w, 3).astype(np.float32)
  gt = feo.disc_labels(rng, N, H, W)
  y_gt = (rng.rand(N, h, w) > 0.5).astype(np.float32)
  d_gt = _one_hot(rng.randint(0, 8, (N, h, w)), 8)
  names = ['a.png', 'b.png', 'c.png']
  src = str(tmp_path / 'in.npz')
  np.savez(src, x=x, fg_gt_full=gt, names=np.array(names), y_gt=y_gt, d_gt=d_gt)
  ref = fo.forward(opt, P, x)
  v64 = feo.upsample(ref['y_out'][..., 0], H, W)
  thr = [0.5, 0.45]
  lo, hi = feo.sweep_counts(v64, gt, thr, +E2E_DELTA), feo.sweep_counts(v64, gt, thr, -E2E_DELTA)
  out = [str(tmp_path / 'out_a'), str(tmp_path / 'out_b')]
  texts = []
  for o in out:
    fg_model_eval.main(['--model_id', 'fg', '--results', res, '--input', src, '--output', o, '--batch_size', '2',
                        '--threshold_list', '0.5,0.45', '--render_soft', '--render_gt'])
    with open(os.path.join(o, 'metrics.yaml')) as f:
      texts.append(f.read())
  assert texts[0] == texts[1]
  met = yaml.safe_load(texts[0])
  assert sorted(met) == ['0.45', '0.50', 'statistics']
  for k, t in enumerate(thr):
    m = met['%.2f' % t]
    print('threshold %.2f: %r; band count_a [%d, %d] sum_ab [%d, %d]' % (t, m, lo[0][:, k].sum(), hi[0][:, k].sum(), lo[1][:, k].sum(),
                                                                         hi[1][:, k].sum()))
    assert lo[0][:, k].sum() <= m['count_a'] <= hi[0][:, k].sum() and lo[1][:, k].sum() <= m['sum_ab'] <= hi[1][:, k].sum()
    assert m['sum_b'] == int(gt.astype(np.int64).sum()) and m['pixels'] == N * H * W
    inter_bg = m['pixels'] - m['count_a'] - m['sum_b'] + m['sum_ab']
    assert m['fg_iou_all'] == m['sum_ab'] / (m['count_a'] + m['sum_b'] - m['sum_ab'])
    assert m['bg_iou_all'] == inter_bg / ((m['pixels'] - m['count_a']) + (m['pixels'] - m['sum_b']) - inter_bg)
    # the analyzers' formulas on the oracle's binary maps at both edges of the band enclose the reported values
    edges = [[(v64[n] > t + s).astype(np.float64) for n in range(N)] for s in (+E2E_DELTA, -E2E_DELTA)]
    gl = [gt[n].astype(np.float64) for n in range(N)]
    if (lo[0][:, k] == hi[0][:, k]).all():
      assert m['fg_iou_all'] == pytest.approx(feo.fg_iou_all(edges[0], gl), rel=1e-14)
      assert m['bg_iou_all'] == pytest.approx(feo.bg_iou_all(edges[0], gl), rel=1e-14)
    else:  # an IoU moves by at most (pixels in the band) * max(gt) / union per unit
      slack = 2.0 * float(gt.max()) * (hi[0][:, k].sum() - lo[0][:, k].sum()) / max(1.0, m['count_a'] + m['sum_b'] - m['sum_ab'])
      assert abs(m['fg_iou_all'] - feo.fg_iou_all(edges[0], gl)) <= slack
    folder = os.path.join(out[0], '%02d' % int(t * 100))
    for n in names:
      img = png.read_gray8(os.path.join(folder, n))
      assert img.shape == (H, W) and set(np.unique(img)) <= {0, 255}
  for sub in ('soft', 'gt'):
    assert png.read_gray8(os.path.join(out[0], sub, 'b.png')).shape == (H, W)
  # the statistics: the mean over the batches (2 + 1 images) of Model.statistics, as the Evaluator averages
  want, bounds = [], []
  for sl in (slice(0, 2), slice(2, 3)):
    part = {k: v[sl] for k, v in ref.items()}
    sums, b = _propagated(part, y_gt[sl], d_gt[sl], 1, 8, float(x[sl].shape[0] * h * w), 'bce')
    want.append(feo.statistics_of(sums, float(x[sl].shape[0] * h * w), 'bce', True))
    bounds.append(b)
  assert sorted(met['statistics']) == sorted(want[0])
  for k, v in met['statistics'].items():
    mean, bound = np.mean([s[k] for s in want]), np.mean([b[k] for b in bounds])
    print('statistics %-16s %.8g (oracle %.8g, propagated bound %.3g)' % (k, v, mean, bound))
    assert abs(v - mean) <= bound + FLOOR
  assert 'fg_iou_all 0.50' in capsys.readouterr().out
