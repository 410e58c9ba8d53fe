"""The wide filter-gradient kernel (csrc/ra_wgrad_wide.hip, ra_conv3x3_wgrad_wide_acc_f32) against _wgrad_ref in float64 at the
project's filter-gradient bar F32_BAR = 2e-5 of max |ref|; float32 torch on the CPU is printed beside it
(profiles/fg_train_wide.txt has both columns).  The cases are the kernel's ragged edges: Cin no multiple of the 64-channel block
(4, 20, 132), Cout a multiple of 16 but not of 64 (144, 272), maps smaller than one 8 x 8 pixel tile or no multiple of it, B = 1,
upsample, the largest block grid (1024 x 512) and one shape whose pixels are split over several workgroups with a short last part."""
import functools

import numpy as np
import pytest
import torch

import ra_ops as ops
from wgrad_form_cases import F32_BAR, _rel, _wgrad_ref

pytestmark = pytest.mark.gpu

# (Cin, Cout, B, Hs, Ws, upsample)
CASES = [(4, 144, 1, 5, 7, 0), (20, 144, 2, 5, 7, 0), (132, 272, 2, 8, 16, 0), (64, 192, 2, 4, 8, 1), (272, 512, 1, 3, 5, 1),
         (1024, 512, 2, 4, 8, 0), (192, 192, 2, 32, 64, 0),
         (144, 144, 3, 24, 24, 0)]  # beyond the issue's list: 27 pixel tiles in 6 parts of 5, the last part short, ragged blocks on both sides


@functools.lru_cache(maxsize=None)
def reference(cin, cout, B, Hs, Ws, ups):
  """-> x, du (float32 host tensors), dW [3,3,cin,cout] and db in float64, float32 torch's error of dW and db.  Computed once."""
  rng = np.random.RandomState(1000 * cin + 10 * cout + Hs + ups)
  up = 1 + ups
  x = torch.from_numpy(rng.randn(B, Hs, Ws, cin).astype(np.float32))
  du = torch.from_numpy(rng.randn(B, Hs * up, Ws * up, cout).astype(np.float32))
  xs = x
  if ups:  # the conv that ran saw x zero-stuffed at the odd positions (wgrad_form_cases._reference)
    xs = torch.zeros((B, 2 * Hs, 2 * Ws, cin))
    xs[:, 1::2, 1::2] = x
  dw, db = _wgrad_ref(xs, du)
  xi = torch.nn.functional.pad(xs, (0, 0, 1, 1, 1, 1))
  H, W = du.shape[1:3]
  dw32 = torch.stack([torch.stack([torch.einsum('bhwc,bhwd->cd', xi[:, ky:ky + H, kx:kx + W], du) for kx in range(3)]) for ky in range(3)])
  return x, du, dw, db, _rel(dw32, dw), _rel(du.sum(dim=(0, 1, 2)), db)


def run(x, du, gw, gb, chan_map=None, transposed=False, ups=0):
  dev = torch.device('cuda')
  cm = None if chan_map is None else torch.tensor(chan_map, dtype=torch.int32, device=dev)
  gw, gb = gw.to(dev), None if gb is None else gb.to(dev)
  ops.wgrad_wide_acc(x.to(dev), du.to(dev), gw, gb, chan_map=cm, transposed=transposed, upsample=bool(ups))
  torch.cuda.synchronize()
  return gw.cpu(), None if gb is None else gb.cpu()


@pytest.mark.parametrize('cin,cout,B,Hs,Ws,ups', CASES)
def test_wide_wgrad_vs_float64(cuda, cin, cout, B, Hs, Ws, ups):
  x, du, dw, db, e32w, e32b = reference(cin, cout, B, Hs, Ws, ups)
  gw, gb = run(x, du, torch.zeros(3, 3, cin, cout), torch.zeros(cout), ups=ups)
  plan = ops.wgrad_wide_plan(cin, cout, B, Hs, Ws, ups)
  ew, eb = _rel(gw, dw), _rel(gb, db)
  print('wgrad_wide %4d -> %3d  B %d  %2d x %2d  ups %d  split %2d x %2d tiles  dW %.3e (float32 torch %.3e)  db %.3e (float32 torch %.3e)  bar %g'
        % (cin, cout, B, Hs, Ws, ups, plan['split'], plan['tiles_per_part'], ew, e32w, eb, e32b, F32_BAR))
  assert torch.isfinite(gw).all() and ew <= F32_BAR and eb <= F32_BAR, (ew, eb)


def test_wide_wgrad_transposed_layout(cuda):
  """[3,3,Cout,cin_w] with flipped taps: a dcnn filter's gradient."""
  cin, cout, B, Hs, Ws, ups = CASES[2]
  x, du, dw, db, _, _ = reference(cin, cout, B, Hs, Ws, ups)
  gw, gb = run(x, du, torch.zeros(3, 3, cout, cin), torch.zeros(cout), transposed=True)
  want = dw.flip(0, 1).permute(0, 1, 3, 2)
  assert _rel(gw, want) <= F32_BAR and _rel(gb, db) <= F32_BAR
  # without a bias bucket nothing else changes
  gw2, none = run(x, du, torch.zeros(3, 3, cout, cin), None, transposed=True)
  assert none is None and torch.equal(gw, gw2)


@pytest.mark.parametrize('transposed', [False, True])
def test_wide_wgrad_accumulates_through_a_channel_map(cuda, transposed):
  """A non-identity chan_map with padding channels, cin_w < Cin, onto a pre-filled bucket: every element has one writer, rows no
  channel maps to keep their value."""
  cin, cout, B, Hs, Ws, ups = CASES[1]  # 20 -> 144
  x, du, dw, db, _, _ = reference(cin, cout, B, Hs, Ws, ups)
  cmap = [3, -1, 0, 1, 2, 17, 4, 5, -1, -1, 6, 7, 8, 9, 10, 16, 11, 12, 13, 14]  # rows 0 .. 14, 16, 17 of 18; row 15 unmapped
  cin_w = 18
  rng = np.random.RandomState(5)
  g0w = torch.from_numpy(rng.randn(*((3, 3, cout, cin_w) if transposed else (3, 3, cin_w, cout))).astype(np.float32))
  g0b = torch.from_numpy(rng.randn(cout).astype(np.float32))
  want = g0w.double().clone()
  for ci, j in enumerate(cmap):
    if j >= 0:
      if transposed:
        want[:, :, :, j] += dw[:, :, ci, :].flip(0, 1)
      else:
        want[:, :, j, :] += dw[:, :, ci, :]
  gw, gb = run(x, du, g0w.clone(), g0b.clone(), chan_map=cmap, transposed=transposed)
  assert _rel(gw, want) <= F32_BAR and _rel(gb, g0b.double() + db) <= F32_BAR
  untouched = gw[:, :, :, 15] if transposed else gw[:, :, 15, :]
  assert torch.equal(untouched, g0w[:, :, :, 15] if transposed else g0w[:, :, 15, :])
  # no map and cin_w < Cin: the first cin_w channels are the filter's rows
  g1, _ = run(x, du, torch.zeros((3, 3, cout, 13) if transposed else (3, 3, 13, cout)), None, transposed=transposed)
  cut = dw[:, :, :13, :]
  assert _rel(g1, cut.flip(0, 1).permute(0, 1, 3, 2) if transposed else cut) <= F32_BAR


def test_wide_wgrad_is_bit_reproducible(cuda):
  cin, cout, B, Hs, Ws, ups = CASES[6]  # the split shape: partial sums from several workgroups
  x, du = reference(cin, cout, B, Hs, Ws, ups)[:2]
  a = run(x, du, torch.zeros(3, 3, cin, cout), torch.zeros(cout))
  b = run(x, du, torch.zeros(3, 3, cin, cout), torch.zeros(cout))
  assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
