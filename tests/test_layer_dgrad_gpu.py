"""ra_layer_train.conv_dgrad, the one data gradient of the training layers, on its own: every route and option against float64
torch.autograd through the oracle's conv / transposed-conv restatements (ra_oracle_torch, train_filter_cases), at B = 2 on a 6 x 10 map, and which route a caller
reaches.  The bars are those of the tests that covered each route through a node before the routes were one function:
  K1 float32, K1s split   2e-3 of max |ref|   test_train_gpu.test_conv_layer_forward_backward (dx)
  k x k                   2e-3 of max |ref|   test_train_filter_sizes_gpu.test_conv_layer_forward_backward_kxk (dx)
  a row range of a filter 2e-5 of max |ref|   test_fg_train_wide_gpu.test_one_layer_through_the_node (dx0 / dx1)
  bf16 operands           2e-3 in relative L2 against the oracle that rounds the same operands
                                              test_train_gpu.test_bf16_conv_layer_vs_emulating_oracle (L2: an operand on a rounding
                                              boundary rounds the other way in float32 than in float64 and moves single elements by 2^-8)
  bf16 storage            the same 2e-3 in L2 against the same oracle with its result rounded to bf16 as the kernel stores it (the
                          'bf16s' oracle of test_train_gpu.test_bf16_storage_step_vs_emulating_oracle); du is drawn bf16-exact, and a
                          result that rounds the other way than the oracle's moves by 2^-8, as above
Run with -s for the measured errors (profiles/layer_dgrad.txt)."""
import numpy as np
import pytest
import torch

import ra_layer_train as lt
import ra_oracle_torch as ort
import ra_ops as ops
import ra_train
import train_filter_cases as tfc
from ra_native import RecAttendError

pytestmark = pytest.mark.gpu

B, HS, WS = 2, 6, 10
BF = torch.bfloat16


def _draw(seed, ksize, rows_w, cout, transposed, stride, bf16_exact=False):
  """w in the reference layout with rows_w input rows, du [B, HS * stride, WS * stride, cout] (float32 host tensors)."""
  rng = np.random.RandomState(seed)
  shape = (ksize, ksize, cout, rows_w) if transposed else (ksize, ksize, rows_w, cout)
  w = torch.from_numpy((rng.randn(*shape) * (0.6 / ksize)).astype(np.float32))
  du = torch.from_numpy(rng.randn(B, HS * stride, WS * stride, cout).astype(np.float32))
  return w, (du.to(BF).float() if bf16_exact else du)


def _reference(w, du, transposed, stride, operands=None):
  """d sum(conv(x) * du) / dx in float64 for x [B,HS,WS,rows of w]: the data gradient towards every filter row."""
  rows_w = w.shape[3] if transposed else w.shape[2]
  x = torch.zeros(B, HS, WS, rows_w, dtype=torch.float64, requires_grad=True)
  zero = torch.zeros(du.shape[3], dtype=torch.float64)
  ort.set_conv_operands(operands)
  try:
    if not transposed:
      u = ort.conv_same(x, w.double(), zero)
    elif w.shape[0] == 3:
      u = ort.deconv_same(x, w.double(), zero, stride)
    else:
      u = tfc.deconv_ref(x, w.double(), zero, stride)
    (u * du.double()).sum().backward()
  finally:
    ort.set_conv_operands(None)
  return x.grad


def _max_rel(got, ref):
  return float((got.detach().cpu().double() - ref).abs().max() / ref.abs().max())


def _l2_rel(got, ref):
  return float(torch.linalg.norm(got.detach().cpu().double() - ref) / torch.linalg.norm(ref))


# name, ksize, filter rows, Cout, transposed, stride, conv_dgrad's options, kernel input channels Cx, bar
F32_CASES = [
    ('8->4 plain', 3, 4, 8, False, 1, {}, 4, 2e-3),
    ('8->4 transposed', 3, 4, 8, True, 1, {}, 4, 2e-3),
    ('5->3 padded to 4', 3, 3, 5, False, 1, {}, 4, 2e-3),
    ('chan_map hole + permutation', 3, 6, 8, False, 1, dict(chan_map=[2, 0, -1, 1, 5, -1, 4, 3]), 8, 2e-3),
    ('stride 2, 3x3', 3, 4, 8, True, 2, {}, 4, 2e-3),
    ('stride 2, 1x1 (even positions)', 1, 4, 8, True, 2, dict(ksize=1), 4, 2e-3),
    ('stride 2, 5x5', 5, 4, 8, True, 2, dict(ksize=5), 4, 2e-3),
    ('5x5 stride 1, 5->3 padded', 5, 3, 5, False, 1, dict(ksize=5), 4, 2e-3),
    ('rows 4..12 of 16', 3, 16, 8, False, 1, dict(rows=(4, 8)), 8, 2e-5),
    ('rows 4..12 of 16, stride 2, padded source', 3, 16, 8, True, 2, dict(rows=(4, 8)), 12, 2e-5),
    ('rows 16..160 of 160 (K1-wide)', 3, 160, 8, False, 1, dict(rows=(16, 144)), 144, 2e-5),
    ('rows 0..144 of 160 (K1-wide), stride 2', 3, 160, 8, True, 2, dict(rows=(0, 144)), 144, 2e-5),
]


@pytest.mark.parametrize('case', F32_CASES, ids=[c[0] for c in F32_CASES])
def test_float32_routes_vs_float64_autograd(cuda, case):
  name, ksize, rows_w, cout, tr, stride, kw, Cx, bar = case
  w, du = _draw(len(name), ksize, rows_w, cout, tr, stride)
  ref = _reference(w, du, tr, stride)
  dud = du.cuda()
  if 'rows' in kw:  # the wide node hands over du with its channels already padded
    dud = lt._pad_channels(dud)
  got = lt.conv_dgrad(dud, w.cuda(), tr, stride, (B, HS, WS, Cx), cache={}, **kw)
  assert tuple(got.shape) == (B, HS, WS, Cx) and got.dtype == torch.float32
  first, n = kw.get('rows', (0, rows_w))
  cmap = kw.get('chan_map', list(range(first, first + n)) + [-1] * (Cx - n))
  real = [c for c, j in enumerate(cmap) if j >= 0]
  err = _max_rel(got[..., real], ref[..., [cmap[c] for c in real]])
  print('dgrad %-64s max rel %.2e (bar %.0e)' % (name, err, bar))
  assert err <= bar
  holes = [c for c, j in enumerate(cmap) if j < 0]
  assert not holes or float(got[..., holes].abs().max()) == 0.0  # padding channels of the kernel input receive exact zeros


@pytest.mark.parametrize('tr,stride', [(False, 1), (True, 2)])
def test_bf16_operands_vs_emulating_oracle(cuda, tr, stride):
  w, du = _draw(11 + stride, 3, 4, 8, tr, stride)
  ref = _reference(w, du, tr, stride, operands='bf16')
  got = lt.conv_dgrad(du.cuda(), w.cuda(), tr, stride, (B, HS, WS, 4), cache={}, bf16=True)
  err, plain = _l2_rel(got, ref), _l2_rel(got, _reference(w, du, tr, stride))
  print('dgrad bf16 operands transposed %d stride %d: L2 rel %.2e vs the emulating oracle (bar 2e-3), %.2e vs unrounded float64' %
        (tr, stride, err, plain))
  assert err <= 2e-3 and err < plain  # closer to ITS oracle than to the unrounded one: the operands were rounded


@pytest.mark.parametrize('tr,stride,du_dt,out_dt', [(False, 1, BF, BF), (True, 2, BF, BF), (False, 1, BF, torch.float32),
                                                     (True, 2, torch.float32, BF)])
def test_bf16_storage_vs_emulating_oracle(cuda, tr, stride, du_dt, out_dt):
  w, du = _draw(17 + stride, 3, 4, 8, tr, stride, bf16_exact=True)
  ref = _reference(w, du, tr, stride, operands='bf16')
  if out_dt == BF:
    ref = ort._bf16_round(ref)
  got = lt.conv_dgrad(du.cuda().to(du_dt), w.cuda(), tr, stride, (B, HS, WS, 4), cache={}, bf16=True, out_dtype=out_dt)
  assert got.dtype == out_dt and tuple(got.shape) == (B, HS, WS, 4)
  err = _l2_rel(got.float(), ref)
  print('dgrad bf16 storage transposed %d stride %d du %s result %s: L2 rel %.2e (bar 2e-3)' % (tr, stride, du_dt, out_dt, err))
  assert err <= 2e-3


def test_more_than_128_rows_without_a_row_range_stay_refused(cuda):
  """K1-wide is the wide node's route alone: a caller that names no row range keeps K1's refusal beyond 128 output channels,
  in float32 and with bf16 operands (160 filter rows, a multiple of 16 that K1-wide would take)."""
  w, du = _draw(3, 3, 160, 8, False, 1)
  for bf16 in (False, True):
    with pytest.raises(RecAttendError, match='unsupported conv shape'):
      lt.conv_dgrad(du.cuda(), w.cuda(), False, 1, (B, HS, WS, 160), cache={}, bf16=bf16)


def _smallest_split_map():
  return min(((h, w) for h in range(1, 33) for w in range(1, 33) if ops.conv_split_supported(32, 32, 1, h, w)), key=lambda hw: (hw[0] * hw[1], hw))


@pytest.mark.parametrize('tr', [False, True])
def test_split_route_is_the_stacked_nodes_alone(cuda, tr):
  """32 -> 32, stride 1, at the smallest map conv_split_supported accepts: conv_dgrad without allow_split IS ops.conv3x3 on the
  flipped pack, with it IS ops.conv_split, bit for bit; ConvBNActPool.backward gives the former (the per-call node does not take
  the split route), ConvStackFn-style calls the latter; both within the float32 bar of float64."""
  H, W = _smallest_split_map()
  rng = np.random.RandomState(5 + tr)
  w = torch.from_numpy((rng.randn(3, 3, 32, 32) * 0.2).astype(np.float32)).cuda()
  du = torch.from_numpy(rng.randn(B, H, W, 32).astype(np.float32)).cuda()
  ones, zeros = lt._ones_zeros(32, du.device)
  k1 = ops.conv3x3(du, lt._pack_dev(w, 32, 32, 32, None, not tr, {}), ones, zeros, 32, relu=False, pool=1)
  k1s = ops.conv_split(du, ops.pack_split_weights_dev(w, 32, 32, transposed=not tr), ones, zeros, 32, relu=False, pool=1)
  assert not torch.equal(k1, k1s)  # two kernels, two summation orders: the equalities below tell the routes apart
  plain = lt.conv_dgrad(du, w, tr, 1, (B, H, W, 32), cache={})
  split = lt.conv_dgrad(du, w, tr, 1, (B, H, W, 32), cache={}, allow_split=True)
  assert torch.equal(plain, k1) and torch.equal(split, k1s)
  # the per-call node, without BatchNorm, ReLU or pool: du is dy itself
  x = torch.zeros(B, H, W, 32, device=du.device, requires_grad=True)
  meta = dict(transposed=tr, stride=1, pool=1, relu=False, chan_map=None, cache={})
  y, _, _ = ra_train.ConvBNActPool.apply(x, w.clone().requires_grad_(True), torch.zeros(32, device=du.device, requires_grad=True), None, None, meta)
  y.backward(du)
  assert torch.equal(x.grad, k1)
  xr = torch.zeros(B, H, W, 32, dtype=torch.float64, requires_grad=True)
  u = ort.deconv_same(xr, w.cpu().double(), torch.zeros(32, dtype=torch.float64), 1) if tr else \
      ort.conv_same(xr, w.cpu().double(), torch.zeros(32, dtype=torch.float64))
  (u * du.cpu().double()).sum().backward()
  errs = _max_rel(plain, xr.grad), _max_rel(split, xr.grad)
  print('dgrad 32->32 at %dx%d transposed %d: K1 max rel %.2e, K1s split %.2e (bar 2e-3)' % (H, W, tr, errs[0], errs[1]))
  assert max(errs) <= 2e-3
