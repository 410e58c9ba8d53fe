"""Float64 parity of the conv kernels in EVERY launch form their host dispatch selects from the problem size.

The tables are in tests/conv_form_cases.py: a case names a shape and the plan (template instantiation, store form, tile walk) it
is meant to reach.  Each case checks that
  1. the plan query, which walks the launch's own chain of choices, returns exactly that plan;
  2. the kernel matches the float64 oracle over every output element, on seeded inputs with a bias, a folded BatchNorm with
     mixed-sign gamma and ReLU, at the bar of that family's test in test_kernels_gpu.py / test_train_gpu.py;
  3. the output, a 16-byte aligned view filled with NaN inside a larger buffer of sentinel words, is written completely and
     nothing outside it is touched (a fresh torch.empty can hand back a previous case's correct result and hide a hole);
  4. a failure reports the worst element's (b, y, x, c) and whether it lies in a ragged last tile.
test_device_plans_are_covered closes the loop for the plans that follow the device's CU count; the device-independent ones are
counted by tests/test_conv_forms_coverage.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import conv_form_cases as cf
import ra_native as rn
import ra_ops as ops
import ra_oracle as ora

pytestmark = pytest.mark.gpu

GUARD = 64            # sentinel floats either side of the output view (256 bytes: the view stays 16-byte aligned)
SENTINEL = 0x4b3c2d1e  # a float32 bit pattern no kernel here computes


def dev(a, cuda):
  return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(cuda)


def bf16_round(a):
  """float32 -> nearest bf16 (ties to even) -> float32: what v_cvt_pk_bf16_f32 does to an operand."""
  return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).bfloat16().float().numpy()


class Guarded(object):
  """An output view filled with NaN between two runs of sentinel words."""

  def __init__(self, shape, cuda):
    n = int(np.prod(shape))
    self.buf = torch.empty(n + 2 * GUARD, dtype=torch.float32, device=cuda)
    self.buf.view(torch.int32).fill_(SENTINEL)
    self.view = self.buf[GUARD:GUARD + n].view(shape)
    self.view.fill_(float('nan'))
    assert self.view.is_contiguous() and self.view.data_ptr() % 16 == 0
    self.n = n

  def result(self, what):
    """The view as numpy, once the sentinels are found bit-identical and the view free of NaN."""
    torch.cuda.synchronize()
    bits = self.buf.view(torch.int32).cpu().numpy()
    lo, hi = bits[:GUARD], bits[GUARD + self.n:]
    assert (lo == SENTINEL).all() and (hi == SENTINEL).all(), '%s: wrote outside its output: %d words before, %d after' % (
        what, int((lo != SENTINEL).sum()), int((hi != SENTINEL).sum()))
    y = self.view.cpu().numpy()
    holes = np.argwhere(np.isnan(y))
    assert len(holes) == 0, '%s: %d output elements never written, first (b, y, x, c) = %s' % (what, len(holes), tuple(int(v) for v in holes[0]))
    return y


def assert_plan(plan, expected, walk=None):
  assert cf.plan_str(plan) == expected, 'the dispatch no longer takes this case to its form: %s' % cf.plan_str(plan)
  if walk is not None:
    got = (plan['ntiles'], plan['grid'], plan['tiles_min'], plan['tiles_max'])
    assert got == walk, 'tile walk (ntiles, grid, fewest, most tiles per workgroup) %r, the case is meant for %r' % (got, walk)


def assert_close(y, ref, bar, plan, pool, what):
  """|y - ref| below bar of the output scale, over every element; the message names the worst one and its tile."""
  assert y.shape == ref.shape, (y.shape, ref.shape)
  err = np.abs(y.astype(np.float64) - ref)
  scale = max(1e-6, np.abs(ref).max())
  b, oy, ox, c = np.unravel_index(int(np.argmax(err)), err.shape)
  e = err[b, oy, ox, c] / scale
  print('%s: %.3g of the output scale (bar %.3g)' % (what, e, bar))
  if e < bar:
    return e
  th, tw = plan['tile_h'], plan['tile_w']
  H, W = ref.shape[1] * pool, ref.shape[2] * pool  # the conv's own rows / columns
  where = '?'
  if th and tw:
    ty, tx = oy * pool // th, ox * pool // tw
    ragged = (H % th and ty == (H - 1) // th, W % tw and tx == (W - 1) // tw)
    where = 'tile (%d, %d) of %d x %d, %s' % (ty, tx, -(-H // th), -(-W // tw),
                                             {(0, 0): 'a full tile', (1, 0): 'the ragged last tile ROW', (0, 1): 'the ragged last tile COLUMN',
                                              (1, 1): 'the ragged CORNER tile'}[(int(bool(ragged[0])), int(bool(ragged[1])))])
  raise AssertionError('%s: %.3g of the output scale >= %.3g at (b, y, x, c) = (%d, %d, %d, %d): got %r, oracle %r; %s; plan %s' % (
      what, e, bar, b, oy, ox, c, float(y[b, oy, ox, c]), float(ref[b, oy, ox, c]), where, cf.plan_str(plan)))


def layer_params(rng, Co):
  """bias, BatchNorm (beta, gamma of mixed sign, mean, var) of one layer, float32."""
  b = (rng.randn(Co) * 0.1).astype(np.float32)
  bn = tuple(a.astype(np.float32) for a in (rng.randn(Co) * 0.2, rng.uniform(0.5, 1.5, Co) * rng.choice([-1, 1], Co), rng.randn(Co) * 0.2,
                                            rng.uniform(0.5, 1.5, Co)))
  return b, bn


def layer_ref(x, w, b, bn, stride=0, relu=True, pool=1):
  """conv (stride 0) or transposed conv (stride 1 | 2) + bias, BatchNorm, ReLU, max-pool in float64."""
  x, w = x.astype(np.float64), w.astype(np.float64)
  r = (ora.conv2d_transpose(x, w, stride) if stride else ora.conv2d(x, w)) + b.astype(np.float64)
  r = ora.batch_norm_eval(r, *[a.astype(np.float64) for a in bn])
  if relu:
    r = ora.relu(r)
  return ora.max_pool(r, pool) if pool > 1 else r


# ------------------------------------------------------------------------------------------------------------------- K1
K1_BARS = {'f32': 2e-5, 'mom': 2e-5, 'k1': 1e-4, 'k5': 1e-4, 'k7': 1e-4}  # test_conv3x3 / test_conv_transpose; test_filter_sizes_gpu


@pytest.mark.parametrize('kind,shape,expected', cf.K1_CASES + cf.K1_EXTRA_CASES,
                         ids=['%s-%s' % (k, 'x'.join(map(str, s))) for k, s, _ in cf.K1_CASES + cf.K1_EXTRA_CASES])
def test_k1_forms(cuda, kind, shape, expected):
  B, Hs, Ws, C0, C1, Co, pool, ups, has_plane = shape
  plan = cf.k1_plan(kind, shape)
  assert_plan(plan, expected)
  kw = cf.K1_KINDS[kind]
  kf, bf16, mom = kw.get('ksize', 3), bool(kw.get('bf16')), bool(kw.get('moments'))
  Cin = C0 + C1
  rng = np.random.RandomState(B * 1000 + Hs * 31 + Ws + Cin + Co + kf)
  x = rng.randn(B, Hs, Ws, Cin).astype(np.float32)
  xr = x.copy()  # what the layer reads
  plane = None
  if has_plane:  # input channel 3 comes from its own plane; the packed image's slot is never read
    plane = rng.randn(B, Hs, Ws).astype(np.float32)
    xr[..., 3] = plane
    x[..., 3] = 777.0
  w = (rng.randn(*((kf, kf, Co, Cin) if ups else (kf, kf, Cin, Co))) / np.sqrt(kf * kf * Cin)).astype(np.float32)
  b, bn = layer_params(rng, Co)
  ref_of = lambda xa, wa, relu=True: layer_ref(xa, wa, b, bn, 2 if ups else 0, relu, pool)
  sc, sh = [dev(a, cuda) for a in ops.fold_bn(b, Co, bn)]
  wp = dev(ops.pack_conv_weights(w, transposed=bool(ups)), cuda)
  x0, x1 = dev(x[..., :C0], cuda), (dev(x[..., C0:], cuda) if C1 else None)
  pl = dev(plane, cuda) if has_plane else None
  Ho, Wo = Hs * (1 + ups) // pool, Ws * (1 + ups) // pool
  out = Guarded((B, Ho, Wo, Co), cuda)
  what = 'K1 %s %r' % (kind, shape)
  if mom:
    part = torch.empty(rn.lib().ra_conv3x3_moments_part_floats(Co), device=cuda)
    nparts, nparts0 = C.c_int(0), C.c_int(0)
    launch = lambda relu, y, n: ops.check(rn.lib().ra_conv3x3_moments_f32(
        ops.ptr(x0), C0, ops.ptr(x1), C1, B, Hs, Ws, ups, ops.ptr(wp), ops.ptr(sc), ops.ptr(sh), Co, relu, int(bf16), ops.ptr(y), ops.ptr(part),
        part.numel(), C.byref(n), rn.stream_ptr()), 'ra_conv3x3_moments_f32')
    u = torch.empty((B, Ho, Wo, Co), device=cuda)
    launch(0, u, nparts0)       # the pre-activation output the moments are taken of ...
    launch(1, out.view, nparts)  # ... and the layer itself; the records of this launch are the ones finished below
    mean, var = torch.empty(Co, device=cuda), torch.empty(Co, device=cuda)
    ops.check(rn.lib().ra_bn_moments_from_partials_f32(ops.ptr(part), nparts.value, Co, ops.ptr(mean), ops.ptr(var), rn.stream_ptr()),
              'ra_bn_moments_from_partials_f32')
  elif bf16:
    ops.conv3x3(x0, wp, sc, sh, Co, relu=True, pool=pool, src1=x1, upsample=bool(ups), out=out.view, plane=pl, plane_chan=3 if has_plane else -1,
                bf16=True)
  else:
    ops.conv2d_fused(x0, wp, sc, sh, Co, kf, relu=True, pool=pool, src1=x1, upsample=bool(ups), out=out.view, plane=pl,
                     plane_chan=3 if has_plane else -1)
  y = out.result(what)
  if bf16:  # test_conv3x3_bf16_operands' two bars: float32 round-off on the rounded operands, the bf16 one on the unrounded
    assert_close(y, ref_of(bf16_round(xr), bf16_round(w)), 2e-5, plan, pool, what + ' vs the oracle on bf16-rounded operands')
    assert_close(y, ref_of(xr, w), 1e-2, plan, pool, what + ' vs the oracle on unrounded operands')
  else:
    assert_close(y, ref_of(xr, w), K1_BARS[kind], plan, pool, what)
  if mom:  # test_conv_epilogue_moments' bars, against float64 moments of the kernel's own pre-activation output
    assert nparts.value > 0 and nparts.value == nparts0.value
    if plan['family'] == 'k1':  # one record per (workgroup, wave row)
      assert nparts.value == plan['grid'] * (4 // plan['wn'])
    assert torch.equal(torch.relu(u), out.view), what + ': the ReLU launch differs from the pre-activation launch'
    ud = u.double().reshape(-1, Co).cpu().numpy()
    rm, rv = ud.mean(axis=0), ud.var(axis=0)
    em, ev = np.abs(mean.cpu().numpy() - rm), np.abs(var.cpu().numpy() - rv)
    assert (em < 1e-5 * np.maximum(np.sqrt(rv), np.abs(rm))).all(), (what, 'mean, worst channel %d' % int(np.argmax(em / np.sqrt(rv))))
    assert (ev < 1e-5 * rv + 1e-9).all(), (what, 'variance, worst channel %d' % int(np.argmax(ev / rv)))


# ---------------------------------------------------------------------------------------------------------- the fused pair
PAIR_ALL = [(s, p, None) for s, p in cf.PAIR_CASES] + cf.PAIR_WALK_CASES


def pair_case(shape, cuda):
  """The seeded inputs of a pair case, on the host and packed on the device, and its float64 oracle (tests/pair_form_digest.py
  walks the same cases with the same bytes)."""
  B, Hs, Ws, Ci, Ca, Cb, ups, pool, has_plane, cache_form = shape
  rng = np.random.RandomState(B * 1000 + Hs * 31 + Ws + Ci + Ca + Cb)
  x = rng.randn(B, Hs, Ws, Ci).astype(np.float32)
  xr = x.copy()
  plane = None
  if has_plane:
    plane = rng.randn(B, Hs, Ws).astype(np.float32)
    xr[..., 3] = plane
    x[..., 3] = 777.0
  wA = (rng.randn(*((3, 3, Ca, Ci) if ups else (3, 3, Ci, Ca))) / np.sqrt(9 * Ci)).astype(np.float32)
  wB = (rng.randn(*((3, 3, Cb, Ca) if ups else (3, 3, Ca, Cb))) / np.sqrt(9 * Ca)).astype(np.float32)
  (bA, bnA), (bB, bnB) = layer_params(rng, Ca), layer_params(rng, Cb)

  def ref_of(xa):
    h = layer_ref(xa, wA, bA, bnA, 2 if ups else 0)
    return layer_ref(h, wB, bB, bnB, 1 if ups else 0, True, pool)
  d = lambda a: dev(a, cuda)
  wpA, wpB = d(ops.pack_conv_weights(wA, transposed=bool(ups))), d(ops.pack_conv_weights(wB, transposed=bool(ups)))
  scA, shA = [d(a) for a in ops.fold_bn(bA, Ca, bnA)]
  scB, shB = [d(a) for a in ops.fold_bn(bB, Cb, bnB)]
  return x, xr, plane, (wpA, scA, shA), (wpB, scB, shB), ref_of


@pytest.mark.parametrize('shape,expected,walk', PAIR_ALL, ids=['x'.join(map(str, c[0])) for c in PAIR_ALL])
def test_pair_forms(cuda, shape, expected, walk):
  B, Hs, Ws, Ci, Ca, Cb, ups, pool, has_plane, cache_form = shape
  plan = cf.pair_plan(shape)
  assert_plan(plan, expected, walk)
  x, xr, plane, (wpA, scA, shA), (wpB, scB, shB), ref_of = pair_case(shape, cuda)
  d = lambda a: dev(a, cuda)
  out = Guarded((B, Hs * (1 + ups) // pool, Ws * (1 + ups) // pool, Cb), cuda)
  what = 'pair %r' % (shape,)
  if cache_form == 0:
    ops.conv_pair(d(x), wpA, scA, shA, Ca, wpB, scB, shB, Cb, poolB=pool, upsampleA=bool(ups), out=out.view, plane=d(plane) if has_plane else None,
                  plane_chan=3 if has_plane else -1)
    assert_close(out.result(what), ref_of(xr), 3e-5, plan, pool, what)
    return
  # the first controller-CNN pair's cached forms: the first timestep (zero canvas) runs the plain N-packed kernel and leaves layer
  # A's image part in the cache; later timesteps read it
  assert ops.first_cache_supported(Ci, Ca, Cb, pool, Hs, Ws)
  zero = torch.zeros((B, Hs, Ws), device=cuda)
  cache = ops.first_cache_alloc(B, Hs, Ws, cuda)
  x0 = xr.copy()
  x0[..., 3] = 0.0
  if cache_form == 1:
    ops.conv_pair_fill_cache(d(x), zero, 3, wpA, scA, shA, wpB, scB, shB, Cb, cache, out.view)
    assert_close(out.result(what), ref_of(x0), 3e-5, plan, pool, what + ' (cache-filling launch)')
    return
  first = torch.empty_like(out.view)
  ops.conv_pair_fill_cache(d(x), zero, 3, wpA, scA, shA, wpB, scB, shB, Cb, cache, first)
  ops.conv_pair_cached(cache, d(plane), 3, wpA, scA, shA, wpB, scB, shB, Cb, out.view)
  assert_close(out.result(what), ref_of(xr), 3e-5, plan, pool, what + ' (cached launch)')


# ------------------------------------------------------------------------------------------------------------------ K1s
SPLIT_ALL = [(s, p, None) for s, p in cf.SPLIT_CASES] + cf.SPLIT_WALK_CASES


@pytest.mark.parametrize('shape,expected,walk', SPLIT_ALL, ids=['x'.join(map(str, c[0])) for c in SPLIT_ALL])
def test_split_forms(cuda, shape, expected, walk):
  B, H, W, Ci, Co, pool, has_plane = shape
  plan = cf.split_plan(shape)
  assert_plan(plan, expected, walk)
  assert ops.conv_split_supported(Ci, Co, pool, H, W)
  rng = np.random.RandomState(B * 1000 + H * 31 + W + Ci + Co)
  x = rng.randn(B, H, W, Ci).astype(np.float32)
  xr = x.copy()
  plane = None
  if has_plane:
    plane = rng.randn(B, H, W).astype(np.float32)
    xr[..., 3] = plane
    x[..., 3] = 777.0
  w = (rng.randn(3, 3, Ci, Co) / np.sqrt(9 * Ci)).astype(np.float32)
  b, bn = layer_params(rng, Co)
  ref = layer_ref(xr, w, b, bn, 0, True, pool)
  sc, sh = [dev(a, cuda) for a in ops.fold_bn(b, Co, bn)]
  pl = dev(plane, cuda) if has_plane else None
  out = Guarded(ref.shape, cuda)
  what = 'K1s %r' % (shape,)
  ops.conv_split(dev(x, cuda), torch.from_numpy(ops.pack_split_weights(w)).to(cuda), sc, sh, Co, relu=True, pool=pool, out=out.view, plane=pl,
                 plane_chan=3 if has_plane else -1)
  y1 = ops.conv3x3(dev(x, cuda), dev(ops.pack_conv_weights(w), cuda), sc, sh, Co, relu=True, pool=pool, plane=pl, plane_chan=3 if has_plane else -1)
  e_split = assert_close(out.result(what), ref, 2e-5, plan, pool, what)
  e_k1 = np.abs(y1.cpu().numpy() - ref).max() / max(1e-6, np.abs(ref).max())
  assert e_split < 4 * e_k1 + 1e-7, (what, e_split, e_k1)  # test_conv_split_precision: at float32 accuracy, K1's on the same inputs


# ------------------------------------------------------------------------------------------- Winograd and its fused pair
WINO_ALL = [(s, p, None) for s, p in cf.WINO_CASES] + cf.WINO_WALK_CASES


@pytest.mark.parametrize('shape,expected,walk', WINO_ALL, ids=['x'.join(map(str, c[0])) for c in WINO_ALL])
def test_winograd_forms(cuda, shape, expected, walk):
  B, H, W, Ci, Co, pool = shape
  plan = cf.wino_plan(shape)
  assert_plan(plan, expected, walk)
  rng = np.random.RandomState(B * 1000 + H * 31 + W + Ci + Co + pool)
  x = rng.randn(B, H, W, Ci).astype(np.float32)
  w = (rng.randn(3, 3, Ci, Co) / np.sqrt(9 * Ci)).astype(np.float32)
  b, bn = layer_params(rng, Co)
  ref = layer_ref(x, w, b, bn, 0, True, pool)
  sc, sh = [dev(a, cuda) for a in ops.fold_bn(b, Co, bn)]
  out = Guarded(ref.shape, cuda)
  what = 'Winograd %r' % (shape,)
  ops.poison_lds()
  ops.conv_wino(dev(x, cuda), dev(ops.pack_wino_weights(w), cuda), sc, sh, Co, relu=True, pool=pool, out=out.view)
  assert_close(out.result(what), ref, 2e-5, plan, pool, what)


PAIR_WINO_ALL = [(s, p, None) for s, p in cf.PAIR_WINO_CASES] + cf.PAIR_WINO_WALK_CASES


@pytest.mark.parametrize('shape,expected,walk', PAIR_WINO_ALL, ids=['x'.join(map(str, c[0])) for c in PAIR_WINO_ALL])
def test_pair_winograd_forms(cuda, shape, expected, walk):
  B, H, W = shape
  plan = cf.pair_wino_plan(shape)
  assert_plan(plan, expected, walk)
  rng = np.random.RandomState(B * 1000 + H * 31 + W)
  x = rng.randn(B, H, W, 8).astype(np.float32)
  wA = (rng.randn(3, 3, 8, 16) / np.sqrt(72)).astype(np.float32)
  wB = (rng.randn(3, 3, 16, 16) / np.sqrt(144)).astype(np.float32)
  (bA, bnA), (bB, bnB) = layer_params(rng, 16), layer_params(rng, 16)
  ref = layer_ref(layer_ref(x, wA, bA, bnA), wB, bB, bnB, 0, True, 2)
  scA, shA = [dev(a, cuda) for a in ops.fold_bn(bA, 16, bnA)]
  scB, shB = [dev(a, cuda) for a in ops.fold_bn(bB, 16, bnB)]
  out = Guarded(ref.shape, cuda)
  what = 'Winograd pair %r' % (shape,)
  ops.poison_lds()
  ops.conv_pair_wino(dev(x, cuda), dev(ops.pack_conv_weights(wA), cuda), scA, shA, dev(ops.pack_wino_weights(wB), cuda), scB, shB, out=out.view)
  assert_close(out.result(what), ref, 2e-5, plan, 2, what)


# ------------------------------------------------------------------------------------------------------------- coverage
def test_device_plans_are_covered(cuda):
  """Host calls only.  Every plan the queries that follow the device's CU count return over the declared grid of shapes — the pair
  with its persistent kernel, K1s, Winograd, the Winograd pair — is the plan of a case above.  No allow-list."""
  from test_conv_forms_coverage import pair_rows
  grid = [(B, H, W) for B in cf.COVER_B for H in cf.COVER_HW for W in cf.COVER_HW if B * H * W <= 1 << 22]
  tables = {
      'conv_pair': (pair_rows(), {p for _, p in cf.PAIR_CASES} | {c[1] for c in cf.PAIR_WALK_CASES}),
      'conv_split': (((B, H, W, ci, co, pool, plane) for B, H, W in grid for ci, co in cf.SPLIT_CHANNELS for pool in (1, 2) for plane in (0, 1)
                      if H % 4 == 0 and W % 4 == 0 and not (plane and ci == 64)),
                     {p for _, p in cf.SPLIT_CASES} | {c[1] for c in cf.SPLIT_WALK_CASES}),
      'conv_wino': (((B, H, W, ci, co, pool) for B, H, W in grid for ci, co in cf.WINO_CHANNELS for pool in (1, 2) if H % 16 == 0 and W % 16 == 0),
                    {p for _, p in cf.WINO_CASES} | {c[1] for c in cf.WINO_WALK_CASES}),
      'conv_pair_wino': (((B, H, W) for B, H, W in grid if H % 16 == 0 and W % 16 == 0),
                         {p for _, p in cf.PAIR_WINO_CASES} | {c[1] for c in cf.PAIR_WINO_WALK_CASES}),
  }
  floor = {'conv_pair': 100, 'conv_split': 26, 'conv_wino': 32, 'conv_pair_wino': 2}  # the grid really spans each dispatch
  uncovered = []
  for name, (rows, cases) in tables.items():
    plans = cf.distinct_plans(name, rows)
    print('%s: %d distinct plans over the grid, %d uncovered' % (name, len(plans), len(plans - cases)))
    assert len(plans) >= floor[name], (name, len(plans))
    uncovered += sorted(plans - cases)
  assert not uncovered, uncovered
