"""Phase A's group map of the N-packed first pair (csrc/ra_conv_pair8.hip, NGeo::cell): 16 interior groups, four strip groups and
a corner group that ONE wave per tile runs (wave tile & 3) cover the 18 rows x 18 pixel pairs layer B reads, each once.  The shapes
are the smallest at which that map can go wrong:

  (1, 16, 32)    one tile: every strip group lies on an image edge
  (1, 6, 18)     the image is smaller than a tile: the strips are wholly outside it and must come out zero
  (2, 18, 34)    8 tiles, all four owners of the corner group; a 2-pixel ragged remainder, so the strips of tile (0, 0) are interior
                 to the image and those of the last tiles straddle its edge
  (3, 50, 70)    ragged both ways, several tile rows: the rows 16 / 17 that a tile shares with the one below
  (225, 18, 34)  900 tiles on 768 workgroups: the persistent walk, the corner's owner changing between a workgroup's tiles

Per shape: the plain pair with 4 and with 8 input channels (canvas plane), the cache-filling launch (zero canvas) and the cached
launch on the cache the fill left, each against the float64 oracle at the bar of tests/test_conv_forms_gpu.py (3e-5 of the output
scale); the fill's cache against ra_conv_first_cache_f32 bit for bit; everything finite (conftest poisons LDS with NaN before
each test)."""
import numpy as np
import pytest
import torch

import conv_form_cases as cf
import ra_ops as ops
import test_conv_forms_gpu as forms

pytestmark = pytest.mark.gpu

SHAPES = [(1, 16, 32), (1, 6, 18), (2, 18, 34), (3, 50, 70), (225, 18, 34)]
BAR = 3e-5  # test_conv_forms_gpu.test_pair_forms


def case4(shape):
  B, H, W = shape
  return (B, H, W, 4, 8, 8, 0, 2, 1, 2)


def in_image_cells(B, H, W):
  """Mask over the cache [B][rows][ngx][pair r][n = p * 8 + co]: the cells of pixels inside the image, (Y, X) at row Y + 1, column
  X = 8 gx - 2 + 2 r + p.  ra_conv_first_cache_f32 writes exactly these; the fill launch may also write cells of its tiles' halo
  outside the image, which no launch reads unmasked."""
  rows, ngx = -(-H // 16) * 16 + 4, -(-W // 32) * 4 + 1
  Y = np.arange(rows) - 1
  X = 8 * np.arange(ngx)[:, None, None] - 2 + 2 * np.arange(4)[None, :, None] + np.arange(2)[None, None, :]  # [gx][r][p]
  m = ((Y >= 0) & (Y < H))[:, None, None, None] & ((X >= 0) & (X < W))[None]
  return np.broadcast_to(m[None, ..., None], (B, rows, ngx, 4, 2, 8)).reshape(B, rows, ngx, 4, 16)


def run_cached_forms(shape, cuda):
  """The fill launch and the cached launch of a shape: (inputs, fill output, cache, cached output, float64 references)."""
  B, H, W = shape
  x, xr, plane, (wpA, scA, shA), (wpB, scB, shB), ref_of = forms.pair_case(case4(shape), cuda)
  d = lambda a: forms.dev(a, cuda)
  zero = torch.zeros((B, H, W), device=cuda)
  cache = ops.first_cache_alloc(B, H, W, cuda)
  first = forms.Guarded((B, H // 2, W // 2, 8), cuda)
  ops.conv_pair_fill_cache(d(x), zero, 3, wpA, scA, shA, wpB, scB, shB, 8, cache, first.view)
  out = forms.Guarded((B, H // 2, W // 2, 8), cuda)
  ops.conv_pair_cached(cache, d(plane), 3, wpA, scA, shA, wpB, scB, shB, 8, out.view)
  return (x, xr, plane, (wpA, scA, shA), (wpB, scB, shB), ref_of), first, cache, out


@pytest.mark.parametrize('shape', SHAPES, ids=['x'.join(map(str, s)) for s in SHAPES])
def test_group_map_forms(cuda, shape):
  B, H, W = shape
  d = lambda a: forms.dev(a, cuda)
  plan = cf.pair_plan(case4(shape))
  assert cf.plan_str(plan).startswith('pair[cached+npacked+split]'), cf.plan_str(plan)
  assert ops.first_cache_supported(4, 8, 8, 2, H, W)
  (x, xr, plane, A, Bp, ref_of), first, cache, out = run_cached_forms(shape, cuda)
  what = 'pair8 groups %r' % (shape,)
  x0 = xr.copy()
  x0[..., 3] = 0.0
  forms.assert_close(first.result(what), ref_of(x0), BAR, plan, 2, what + ' (cache-filling launch)')
  forms.assert_close(out.result(what), ref_of(xr), BAR, plan, 2, what + ' (cached launch)')
  # the fill's cache = the cache kernel's, bit for bit, wherever a pixel of the image lives
  want = ops.first_cache_alloc(B, H, W, cuda)
  ops.first_cache(d(x), A[0], 8, 3, want)
  torch.cuda.synchronize()
  got_c, want_c = cache.cpu().numpy(), want.cpu().numpy()
  assert np.isfinite(got_c).all(), what + ': the fill left a non-finite value in the cache'
  cells = in_image_cells(B, H, W).reshape(-1)
  assert cells.sum() == B * H * W * 8
  differ = np.flatnonzero((got_c.view(np.int32) != want_c.view(np.int32)) & cells)
  assert len(differ) == 0, '%s: %d cache floats differ from ra_conv_first_cache_f32, first at float %d' % (what, len(differ), differ[0])
  # the plain pair, 4 channels (this case's inputs) and 8 channels (a case of its own), canvas plane in channel 3
  for Ci in (4, 8):
    shp = (B, H, W, Ci, 8, 8, 0, 2, 1, 0)
    pl = cf.pair_plan(shp)
    assert cf.plan_str(pl).startswith('pair[npacked] ck%d' % Ci), cf.plan_str(pl)
    xi, xri, pli, (wpA, scA, shA), (wpB, scB, shB), ref_i = forms.pair_case(shp, cuda)
    o = forms.Guarded((B, H // 2, W // 2, 8), cuda)
    ops.conv_pair(d(xi), wpA, scA, shA, 8, wpB, scB, shB, 8, poolB=2, out=o.view, plane=d(pli), plane_chan=3)
    y = o.result(what)
    assert np.isfinite(y).all()
    forms.assert_close(y, ref_i(xri), BAR, pl, 2, what + ' (plain, %d channels)' % Ci)


def test_corner_owner_with_tile_tickets(cuda):
  """The wave that runs a tile's corner group follows the TILE's index, so drawn tiles (ra_tile_tickets_bind) give the bits of the
  static walk.  (2304 tiles is the first count at which this launch draws, 3 tiles per workgroup on 768: the two smaller shapes
  keep the static walk with tickets bound, and must not be disturbed by them.)"""
  for shape in ((225, 18, 34), (2, 18, 34), (576, 18, 34)):
    B, H, W = shape
    plan = cf.pair_plan(case4(shape))
    assert plan['tickets'] == (1 if B == 576 else 0), (shape, plan)
    (x, xr, plane, (wpA, scA, shA), (wpB, scB, shB), ref_of), first, cache, out = run_cached_forms(shape, cuda)
    ref = torch.from_numpy(out.result('static walk %r' % (shape,))).to(cuda)
    tk = ops.tickets_alloc(4, cuda)
    if not ops.tickets_bind(tk):
      pytest.skip('tile tickets are not available on this device (XCC census)')
    try:
      got = [ops.conv_pair_cached(cache, forms.dev(plane, cuda), 3, wpA, scA, shA, wpB, scB, shB, 8, torch.empty_like(ref)) for _ in range(2)]
    finally:
      ops.tickets_unbind()
    torch.cuda.synchronize()
    for g in got:
      assert torch.equal(g.view(torch.int32), ref.view(torch.int32)), shape
    assert bool((tk.view(torch.int32) != 0).any()) == (B == 576), shape
