"""Train-mode BatchNorm for any C % 4 == 0 up to 512 (csrc/ra_bn_wide.hip) against the float64 references of
tests/bn_form_cases.py at its BARS, with its normalisations: moments absolute on randn * 2 + 3, forward relative to max |y|,
du / dgamma / dbeta relative to max(1, max |.|).  C / 4 = 33 and 48 are no powers of two, 512 is beyond ra_bn.hip's moments;
(1, 2, 2) is one pooled window, (2, 6, 10) a ragged last round of windows, (3, 20, 20) several records per channel."""
import functools

import numpy as np
import pytest
import torch

import bn_form_cases as bfc
import ra_native as rn
import ra_ops as ops

pytestmark = pytest.mark.gpu

CHANNELS = (132, 192, 256, 512)
SHAPES = ((1, 2, 2), (2, 6, 10), (3, 20, 20))


@functools.lru_cache(maxsize=None)
def case_inputs(C_, shape):
  """Group 0 of bn_form_cases.inputs at the first seed without a tied pool maximum (the oracle and the kernel route dy to the
  first maximum; a float32 tie would let them disagree for no fault of either)."""
  for seed in range(16):
    u, dy, gamma, beta, mean, var = bfc.inputs(dict(C=C_, shape=shape, seed=seed))
    if bfc.pool_ties(u[0]) == 0:
      return u[0], {p: dy[p][0] for p in dy}, gamma[0], beta[0], mean[0], var[0]
  raise AssertionError('no seed without pool ties')


def _dev(a):
  return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _err(got, ref, rel_to_max=False):
  ref = np.asarray(ref)
  scale = np.abs(ref).max() if rel_to_max else max(1.0, np.abs(ref).max())
  return float(np.abs(got.cpu().numpy().astype(np.float64) - ref).max() / scale)


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('C_', CHANNELS)
def test_bn_wide_vs_float64(cuda, C_, shape):
  u, dy, gamma, beta, mean, var = case_inputs(C_, shape)
  B, H, W = shape
  ud, gd, bd, md, vd = _dev(u), _dev(gamma), _dev(beta), _dev(mean), _dev(var)
  m, v = ops.bn_wide_moments(ud)
  m2, v2 = ops.bn_wide_moments(ud)
  f64 = u.astype(np.float64).reshape(-1, C_)
  em, ev = float(np.abs(m.cpu().numpy() - f64.mean(0)).max()), float(np.abs(v.cpu().numpy() - f64.var(0)).max())
  print('bn_wide C %3d %s: mean %.3e var %.3e' % (C_, shape, em, ev))
  assert em <= bfc.BARS['mean'] and ev <= bfc.BARS['var']
  assert torch.equal(m, m2) and torch.equal(v, v2)
  if C_ <= 256:  # ra_bn_moments_f32's own range: the two kernels agree to the same bar
    ws = torch.empty(rn.lib().ra_bn_workspace_floats(C_), device='cuda')
    m0, v0 = torch.empty(C_, device='cuda'), torch.empty(C_, device='cuda')
    rn.check(rn.lib().ra_bn_moments_f32(rn.ptr(ud), B * H * W, C_, rn.ptr(ws), ws.numel(), rn.ptr(m0), rn.ptr(v0), rn.stream_ptr()), 'moments')
    assert float((m - m0).abs().max()) <= bfc.BARS['mean'] and float((v - v0).abs().max()) <= bfc.BARS['var']
  for pool in (1, 2):
    dyd = _dev(dy[pool])
    for relu in (0, 1):
      y = ops.bn_wide_act_pool(ud, md, vd, gd, bd, relu=relu, pool=pool)
      ef = _err(y, bfc._fwd_ref(u, mean, var, gamma, beta, relu, pool), rel_to_max=True)
      # accumulation into pre-filled buckets; the plain sums come back beside them
      acc_g, acc_b = torch.full((C_,), 2.0, device='cuda'), torch.full((C_,), -3.0, device='cuda')
      du, dg, db = ops.bn_wide_act_pool_bwd(ud, dyd, md, vd, gd, bd, relu=relu, pool=pool, acc_gamma=acc_g, acc_beta=acc_b)
      rdu, rdg, rdb = bfc._bn_bwd_ref(u, dy[pool], None, None, gamma, beta, relu, pool, bfc.EPS)
      e = dict(fwd=ef, du=_err(du, rdu), dgamma=_err(dg, rdg), dbeta=_err(db, rdb))
      print('  pool %d relu %d: %s' % (pool, relu, '  '.join('%s %.3e' % kv for kv in e.items())))
      for k, val in e.items():
        assert val <= bfc.BARS[k], (k, pool, relu, val)
      assert torch.equal(acc_g, dg + 2.0) and torch.equal(acc_b, db - 3.0)
      # bit-equal repeats, with and without buckets
      du2, dg2, db2 = ops.bn_wide_act_pool_bwd(ud, dyd, md, vd, gd, bd, relu=relu, pool=pool)
      assert torch.equal(du, du2) and torch.equal(dg, dg2) and torch.equal(db, db2)
      assert torch.equal(y, ops.bn_wide_act_pool(ud, md, vd, gd, bd, relu=relu, pool=pool))


def test_bn_wide_without_statistics(cuda):
  """mean / var / gamma / beta absent (use_bn False): y = pool(relu(u)) and du = dy routed through pool and ReLU."""
  u, dy, _, _, _, _ = case_inputs(132, (2, 6, 10))
  ud, dyd = _dev(u), _dev(dy[2])
  y = ops.bn_wide_act_pool(ud, None, None, None, None, relu=1, pool=2)
  ut = torch.tensor(u, requires_grad=True)
  ref = torch.nn.functional.max_pool2d(torch.relu(ut).permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)
  assert torch.equal(y.cpu(), ref.detach())
  (ref * torch.tensor(dy[2])).sum().backward()
  du, _, _ = ops.bn_wide_act_pool_bwd(ud, dyd, None, None, None, None, relu=1, pool=2)
  assert torch.equal(du.cpu(), ut.grad)
