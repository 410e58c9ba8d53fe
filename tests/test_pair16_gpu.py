"""K1p16 (csrc/ra_conv_pair16.hip, ra_conv_pair16_f32): the fused pair 8 -> 16 -> 16, pool 2, with both layers direct on the bf16
matrix pipe.  Against the float64 oracle and against ops.conv_pair (the float32 direct pair) on the same inputs, at the bar the
project holds this pair to (2e-5 of the output scale: test_pair_winograd_forms, test_conv_pair_winograd); folded BatchNorm scales
of random sign; everything finite with LDS poisoned before each launch; guard bands intact.  The shapes are the smallest at which
the kernel can go wrong:

  (1, 16, 16)   one tile column, two tile rows: every window edge on the image border, window rows shared between the two tiles
                (also once without either ReLU)
  (2, 32, 48)   4 x 3 tiles with a fully interior tile (its halo entirely inside the image); two images, for the batch stride
  (B, 16, 80)   the smallest B for which the plan reports more tiles than workgroups: the persistent walk
  (B, 16, 16)   the smallest B at which the plan draws tiles as tickets, and one below it: the bits of the static walk

and one engine forward at the CVPPP arch with the form on and off."""
import numpy as np
import pytest
import torch

import ra_ops as ops
import ra_oracle as ora
import test_conv_forms_gpu as forms

pytestmark = pytest.mark.gpu

BAR = 2e-5  # test_conv_forms_gpu.test_pair_winograd_forms, test_kernels_gpu.test_conv_pair_winograd
MASK_TOL = 1e-3  # tests/test_full_model_gpu.py


def first_B(H, W, pred, limit=1 << 14):
  """The smallest batch at which the plan of (B, H, W) satisfies pred.  Host calls only."""
  for B in range(1, limit):
    if pred(ops.conv_pair16_plan(B, H, W)):
      return B
  raise AssertionError('no batch below %d reaches the plan' % limit)


def case(shape, cuda, relu=True, oracle=True):
  """Seeded inputs of a shape on the device, the float64 reference (oracle=False: none) and the float32 direct pair's output."""
  B, H, W = shape
  rng = np.random.RandomState(B * 1000 + H * 31 + W)
  x = rng.randn(B, H, W, 8).astype(np.float32)
  wA = (rng.randn(3, 3, 8, 16) / np.sqrt(72)).astype(np.float32)
  wB = (rng.randn(3, 3, 16, 16) / np.sqrt(144)).astype(np.float32)
  (bA, bnA), (bB, bnB) = forms.layer_params(rng, 16), forms.layer_params(rng, 16)  # gamma of mixed sign
  ref = forms.layer_ref(forms.layer_ref(x, wA, bA, bnA, 0, relu), wB, bB, bnB, 0, relu, 2) if oracle else None
  d = lambda a: forms.dev(a, cuda)
  scA, shA = [d(a) for a in ops.fold_bn(bA, 16, bnA)]
  scB, shB = [d(a) for a in ops.fold_bn(bB, 16, bnB)]
  args = (d(x), d(ops.pack_conv_weights(wA)), scA, shA, d(ops.pack_conv_weights(wB)), scB, shB)
  xd, wpa, _, _, wpb, _, _ = args
  direct = ops.conv_pair(xd, wpa, scA, shA, 16, wpb, scB, shB, 16, reluA=relu, reluB=relu, poolB=2)
  torch.cuda.synchronize()
  return args, ref, direct.cpu().numpy().astype(np.float64)


def run_checked(shape, cuda, relu=True):
  B, H, W = shape
  assert ops.conv_pair16_supported(8, 16, 16, 2, H, W) and not ops.conv_pair16_supported(8, 16, 16, 1, H, W)
  plan = ops.conv_pair16_plan(B, H, W)
  args, ref, direct = case(shape, cuda, relu)
  out = forms.Guarded((B, H // 2, W // 2, 16), cuda)
  what = 'direct bf16 pair %r%s' % (shape, '' if relu else ' without ReLU')
  ops.poison_lds()
  ops.conv_pair16(*args, reluA=relu, reluB=relu, out=out.view)
  y = out.result(what)
  assert np.isfinite(y).all(), what
  forms.assert_close(y, ref, BAR, plan, 2, what + ' vs float64')
  forms.assert_close(y, direct, BAR, plan, 2, what + ' vs the float32 direct pair')
  return plan


@pytest.mark.parametrize('shape,relu', [((1, 16, 16), True), ((1, 16, 16), False), ((2, 32, 48), True)],
                         ids=['1x16x16', '1x16x16-norelu', '2x32x48'])
def test_pair16_small_shapes(cuda, shape, relu):
  plan = run_checked(shape, cuda, relu)
  assert plan['ntiles'] == plan['grid'] == shape[0] * (shape[1] // 8) * (shape[2] // 16)


def test_pair16_persistent_walk(cuda):
  B = first_B(16, 80, lambda p: p['ntiles'] > p['grid'])
  plan = run_checked((B, 16, 80), cuda)
  assert plan['tiles_max'] >= 2 and plan['tickets'] == 0, plan


def test_pair16_tile_tickets_give_the_static_walks_bits(cuda):
  """Drawn tiles (ra_tile_tickets_bind) give the bits of the static walk; the shape one below the threshold keeps the static walk
  with tickets bound and must not be disturbed by them."""
  Bt = first_B(16, 16, lambda p: p['tickets'] == 1)
  for B in (Bt, Bt - 1):
    plan = ops.conv_pair16_plan(B, 16, 16)
    assert plan['tickets'] == (1 if B == Bt else 0), (B, plan)
    args, _, direct = case((B, 16, 16), cuda, oracle=False)
    out = forms.Guarded((B, 8, 8, 16), cuda)
    ops.poison_lds()
    ops.conv_pair16(*args, out=out.view)
    y = out.result('static walk, B = %d' % B)
    forms.assert_close(y, direct, BAR, plan, 2, 'static walk, B = %d, vs the float32 direct pair' % B)
    ref = torch.from_numpy(y).to(cuda)
    tk = ops.tickets_alloc(4, cuda)
    if not ops.tickets_bind(tk):
      pytest.skip('tile tickets are not available on this device (XCC census)')
    try:
      got = [ops.conv_pair16(*args, out=torch.empty_like(ref)) for _ in range(2)]
    finally:
      ops.tickets_unbind()
    torch.cuda.synchronize()
    for g in got:
      assert torch.equal(g.view(torch.int32), ref.view(torch.int32)), B
    assert bool((tk.view(torch.int32) != 0).any()) == (B == Bt), B


def test_pair16_plan_record(cuda):
  """Host calls only: family, form, tile, tiles and grid of the plan at the shapes above.  The grid is the resident workgroups —
  three per CU, which the kernel's 49920 bytes of LDS allow — or the tiles where those are fewer."""
  resident = 3 * torch.cuda.get_device_properties(cuda).multi_processor_count
  Bw = first_B(16, 80, lambda p: p['ntiles'] > p['grid'])
  Bt = first_B(16, 16, lambda p: p['tickets'] == 1)
  assert Bw == resident // 10 + 1 and Bt == 3 * resident  # more tiles than workgroups; six tiles per workgroup
  for B, H, W in ((1, 16, 16), (2, 32, 48), (Bw, 16, 80), (Bt - 1, 16, 16), (Bt, 16, 16)):
    p = ops.conv_pair16_plan(B, H, W)
    ntiles = B * (H // 8) * (W // 16)
    assert p['family'] == 'pair' and p['form'] == ('persist', 'split'), p
    assert (p['ck'], p['cmid'], p['nc'], p['kf'], p['pool'], p['slices']) == (8, 16, 1, 3, 2, 1), p
    assert (p['tile_h'], p['tile_w'], p['tiles_x'], p['tiles_y']) == (8, 16, W // 16, H // 8), p
    assert (p['ntiles'], p['grid']) == (ntiles, min(ntiles, resident)), p
    assert p['xcd_map'] == (1 if p['grid'] % 8 == 0 else 0) and p['tickets'] == (1 if B == Bt else 0), p
  with pytest.raises(Exception):
    ops.conv_pair16_plan(1, 16, 24)  # W % 16


def test_engine_forward_agrees_with_and_without_pair16(cuda, monkeypatch):
  """A DecodeEngine forward at the CVPPP arch, 64 x 64, T = 2, B = 2, with pair_direct16 on and off: the on run launches the
  new form, the off run does not, and the two agree to the bar of tests/test_full_model_gpu.py."""
  import full_model
  opt = ora.make_opt('cvppp', 64, 64, 2)
  P = ora.random_params(opt, 29)
  x = np.random.RandomState(30).rand(2, 64, 64, 3).astype(np.float32)
  calls = []
  real = ops.conv_pair16
  monkeypatch.setattr(ops, 'conv_pair16', lambda *a, **k: (calls.append(1), real(*a, **k))[1])
  outs = {}
  for on in (True, False):
    m = full_model.get_model(opt).load_weights(P)
    m.engine.pair_direct16 = on
    m.engine.use_graph = False
    del calls[:]
    outs[on] = m.run(['y_out', 's_out'], {'x': x, 'phase_train': False}, as_numpy=True)
    assert (len(calls) > 0) == on, (on, len(calls))
  for u, v in zip(outs[True], outs[False]):
    assert u.shape == v.shape and np.isfinite(u).all()
    assert np.abs(u - v).max() < MASK_TOL, np.abs(u - v).max()
