"""The train-mode BatchNorm kernels (csrc/ra_bn.hip) in every form their host chooser selects: one table of cases, one runner.

A case is a channel count and a shape (B, H, W), the smallest that reaches a path (the comment beside it says which), with the
form ra_bn_form must report for each pass there: literals read off the chooser's rules, asserted by tests/test_bn_forms_gpu.py.
Every case runs, on G = 3 groups of seeded host inputs (u = randn * 2 + 3):
  moments                               against float64
  forward, relu 0 / 1 x pool 1 / 2      against float64
  backward per call, the same four      plain and accumulating (the bucket must equal the returned sums), against _bn_bwd_ref;
    split                               reduce then dx with n_total = 0: the fused call's bits where both run the same form (a
                                        fused `small` call sums in another order than the split generic kernels: those meet
                                        the oracle's bars instead); dx with n_total = 2 B H W against the oracle at that count
    grouped                             the G groups in one call: the bits of the G per-call results, buckets included
  bf16 storage (flags 1 and 3; v4 only) on bf16-exact inputs: du and y equal the float32 kernels' rounded to bf16, sums bit-equal
  refusals                              where the chooser reports an error the entry point returns that code and writes nothing

  python tests/bn_form_cases.py [--lib SO]

prints one line per case:  case NAME FORMS SHA256 err:bar ...  FORMS = moments/forward/backward/split/grouped as ra_bn_form
reports them ('-' from a library without the query), SHA256 over every output byte of the case.  Inputs come from a seeded NumPy
generator on the host and no kernel uses atomics, so two builds of the library must print the same digests (tools/bn_digest.py
compares them without the FORMS column).

The oracle routes dy to the first maximum of a pool window in row-major order, as the kernels do; a window whose maximum is
attained twice in float32 would still let the two disagree for no fault of either, so pool_ties() counts such windows on the
host and the runner requires none (the seeds below were chosen so)."""
import ctypes as C
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(ROOT, 'rec-attend-public_amd') not in sys.path:
  sys.path.insert(0, os.path.join(ROOT, 'rec-attend-public_amd'))

VARIANTS = {'A': {}}  # no variable selects a form: tools/wgrad_digest.py's driver runs the table once
G = 3
EPS = 1e-3
E_SHAPE = -2  # RA_E_SHAPE

# The project's bars at the small shapes (tests/test_train_small_gpu.py, tests/test_train_gpu.py): moments absolute on
# randn * 2 + 3, forward relative to max |y|, du / dgamma / dbeta relative to max(1, max |.|).
BARS = dict(mean=8e-6, var=4e-5, fwd=1e-4, du=2e-5, dgamma=1e-4, dbeta=1e-4)
# At the three large shapes nobody had measured the float32 summation error: each bar is 4 x the error of the build of commit
# a767bc5 (before the kernels moved to ra_bn.hip) against the float64 oracle, the margin being for other seeds.  Measured
# errors, in BARS' order, are in profiles/bn_forms.txt.
LARGE_BARS = {  # quantity: 4 x the measured error (the comment after each line)
    'C8@3x192x16': dict(mean=1.13e-06, var=1.83e-06, fwd=5.22e-07, du=4.97e-07, dgamma=6.71e-07, dbeta=4.24e-07),
        # measured 2.823e-07 4.570e-07 1.305e-07 1.242e-07 1.677e-07 1.059e-07
    'C8@2x192x192': dict(mean=8.68e-07, var=1.38e-06, fwd=5.35e-07, du=7.19e-07, dgamma=5.46e-07, dbeta=5.85e-07),
        # measured 2.171e-07 3.446e-07 1.338e-07 1.797e-07 1.366e-07 1.463e-07
    'C1@2x192x192': dict(mean=6.83e-07, var=1.20e-06, fwd=2.99e-07, du=5.47e-07, dgamma=7.75e-06, dbeta=2.76e-06),
        # measured 1.708e-07 2.998e-07 7.475e-08 1.367e-07 1.938e-06 6.888e-07
    'C96@3x20x20': dict(mean=1.28e-06, var=2.64e-06, fwd=4.22e-07, du=7.13e-07, dgamma=5.50e-07, dbeta=4.55e-07),
        # measured 3.197e-07 6.588e-07 1.054e-07 1.782e-07 1.375e-07 1.137e-07
}


def _case(C_, shape, moments, forward, backward, split, grouped, seed=0):
  """forms expected from ra_bn_form: moments, forward, per-call backward (stages 3), its split stages, grouped (G groups)"""
  return dict(name='C%d@%s' % (C_, 'x'.join(map(str, shape))), C=C_, shape=shape, seed=seed,
              forms=(moments, forward, backward, split, grouped))


CASES = [
    # v4 with ragged rows: B H = 18 rows against 4 per iteration unpooled, 9 pooled
    _case(4, (3, 6, 10), 'small', 'v4', 'v4', 'v4', 'v4'),
    _case(8, (3, 6, 10), 'small', 'v4', 'v4', 'v4', 'v4'),
    # v4 with gx = 3 (pool 1) and gx = 2 (pool 2): dead lanes in the last block of a row
    _case(64, (2, 6, 36), 'small', 'v4', 'v4', 'v4', 'v4'),
    # the upper end of v4: sum_by_group without a shuffle step
    _case(256, (1, 4, 6), 'v4', 'v4', 'v4', 'v4', 'v4'),
    # v4 reduce row stride (576 rows > 512 workgroups); v4 moments (73728 values > 65536)
    _case(8, (3, 192, 16), 'v4', 'v4', 'v4', 'v4', 'v4'),
    # v4 moments grid stride (147456 float4s > 131072); at C = 1 the generic kernels above the one-workgroup limit
    _case(8, (2, 192, 192), 'v4', 'v4', 'v4', 'v4', 'v4'),
    _case(1, (2, 192, 192), 'generic', 'generic', 'generic', 'generic', E_SHAPE),
    # the moments' small / v4 boundary: exactly 65536 values, then one column more
    _case(8, (2, 64, 64), 'small', 'v4', 'v4', 'v4', 'v4'),
    _case(8, (2, 64, 66), 'v4', 'v4', 'v4', 'v4', 'v4'),
    # small: moments and backward (the one-channel output layer)
    _case(1, (8, 48, 48), 'small', 'generic', 'small', 'generic', 'small'),
    # small with pooling; at C = 16 only the moments are small
    _case(2, (3, 10, 12), 'small', 'generic', 'small', 'generic', 'small'),
    _case(16, (2, 6, 6), 'small', 'v4', 'v4', 'v4', 'v4'),
    # generic with idle threads (256 mod C != 0)
    _case(3, (3, 6, 10), 'generic', 'generic', 'generic', 'generic', E_SHAPE),
    _case(12, (3, 6, 10), 'generic', 'generic', 'generic', 'generic', E_SHAPE),
    # generic with 2 pixel lanes and a grid stride (1200 pixels > 1024); bf16 storage and the grouped call are refused
    _case(96, (3, 20, 20), 'generic', 'generic', 'generic', 'generic', E_SHAPE),
]


def _bn_bwd_ref(u, dy, mean, var, gamma, beta, relu, pool, eps=1e-3, n_total=None):
  """float64: y = pool(relu(gamma * (u - mean) * rstd + beta)) with the batch statistics as functions of u -> du, dgamma,
  dbeta.  n_total: du for sums that were taken over n_total values per channel instead (this call's dgamma / dbeta stand for
  the whole data-parallel batch's: the dx stage's formula)."""
  ut = torch.tensor(u, dtype=torch.float64, requires_grad=True)
  g, b = torch.tensor(gamma, dtype=torch.float64, requires_grad=True), torch.tensor(beta, dtype=torch.float64, requires_grad=True)
  C_ = u.shape[-1]
  flat = ut.reshape(-1, C_)
  mu, vv = flat.mean(0), flat.var(0, unbiased=False)
  xhat = (ut - mu) / torch.sqrt(vv + eps)
  v = pre = xhat * g + b
  pre.retain_grad()
  if relu:
    v = torch.relu(v)
  if pool == 2:
    v = torch.nn.functional.max_pool2d(v.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)
  (v * torch.tensor(dy, dtype=torch.float64)).sum().backward()
  du = ut.grad
  if n_total is not None:
    dv, xh = pre.grad, xhat.detach()
    du = g.detach() / torch.sqrt(vv.detach() + eps) * (dv - b.grad / n_total - xh * g.grad / n_total)
  return du.numpy(), g.grad.numpy(), b.grad.numpy()


def _fwd_ref(u, mean, var, gamma, beta, relu, pool):
  v = torch.tensor(gamma, dtype=torch.float64) * (torch.tensor(u, dtype=torch.float64) - torch.tensor(mean, dtype=torch.float64)) / torch.sqrt(
      torch.tensor(var, dtype=torch.float64) + EPS) + torch.tensor(beta, dtype=torch.float64)
  if relu:
    v = torch.relu(v)
  if pool == 2:
    v = torch.nn.functional.max_pool2d(v.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)
  return v.numpy()


def pool_ties(u):
  """2 x 2 pool windows of u [..., H, W, C] (float32) whose maximum is attained more than once."""
  H, W, C_ = u.shape[-3:]
  w = np.sort(u.reshape(-1, H // 2, 2, W // 2, 2, C_).transpose(0, 1, 3, 5, 2, 4).reshape(-1, 4), axis=1)
  return int((w[:, 3] == w[:, 2]).sum())


def inputs(case):
  """The host inputs of a case: u [G,B,H,W,C], dy[pool] [G,B,H/pool,W/pool,C], gamma / beta / mean / var [G,C] (the statistics
  are u's own, taken in float64)."""
  B, H, W = case['shape']
  C_ = case['C']
  rng = np.random.RandomState(1000 * C_ + H + W + case['seed'])
  u = (rng.randn(G, B, H, W, C_) * 2.0 + 3.0).astype(np.float32)
  dy = {p: rng.randn(G, B, H // p, W // p, C_).astype(np.float32) for p in (1, 2)}
  gamma, beta = rng.uniform(0.5, 1.5, (G, C_)).astype(np.float32), (0.2 * rng.randn(G, C_)).astype(np.float32)
  flat = u.astype(np.float64).reshape(G, -1, C_)
  return u, dy, gamma, beta, flat.mean(1).astype(np.float32), flat.var(1).astype(np.float32)


def bars_of(case):
  return dict(BARS, **LARGE_BARS.get(case['name'], {}))


def reported_forms(lib, case):
  """ra_bn_form's answers for the five calls of a case, as the table spells them; None from a library without the query."""
  if not hasattr(lib, 'ra_bn_form'):
    return None
  import ra_ops as ops
  (B, H, W), C_ = case['shape'], case['C']
  return (ops.bn_form('moments', C_, B, H, W), ops.bn_form('forward', C_, B, H, W), ops.bn_form('backward', C_, B, H, W),
          ops.bn_form('backward', C_, B, H, W, stages=1), ops.bn_form('backward', C_, B, H, W, G=G))


def run_case(lib, rn, case, dev):
  """Runs one case; returns (sha256 of all output bytes, [(what, err, bar), ...], [a line per broken relation])."""
  (B, H, W), C_ = case['shape'], case['C']
  f_mom, f_fwd, f_bwd, f_split, f_grp = case['forms']
  u, dy, gamma, beta, mean, var = inputs(case)
  bars, errs, bad, sha = bars_of(case), [], [], hashlib.sha256()
  p, st = rn.ptr, rn.stream_ptr
  dv = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
  new = lambda *s: torch.full(s, float('nan'), device=dev)
  nbn = lib.ra_bn_workspace_floats(C_)

  def out(*ts):
    torch.cuda.synchronize()
    for t in ts:
      sha.update((t.float() if t.dtype == torch.bfloat16 else t).cpu().numpy().tobytes())

  def err(what, got, ref, rel_to_max=False):
    ref = np.asarray(ref)
    scale = np.abs(ref).max() if rel_to_max else max(1.0, np.abs(ref).max())
    errs.append((what, float(np.abs(got.cpu().numpy().astype(np.float64) - ref).max() / scale), bars[what.split('.')[0]]))

  def same(what, a, b):
    if not all(torch.equal(x, y) for x, y in zip(a, b)):
      bad.append(what)

  Ud, Gd, Bd, Md, Vd = dv(u), dv(gamma), dv(beta), dv(mean), dv(var)
  # ---- moments (group 0) ----
  ws, m, v = new(nbn), new(C_), new(C_)
  rn.check(lib.ra_bn_moments_f32(p(Ud[0]), B * H * W, C_, p(ws), nbn, p(m), p(v), st()), 'moments')
  out(m, v)
  f64 = u[0].astype(np.float64).reshape(-1, C_)
  errs.append(('mean', float(np.abs(m.cpu().numpy() - f64.mean(0)).max()), bars['mean']))
  errs.append(('var', float(np.abs(v.cpu().numpy() - f64.var(0)).max()), bars['var']))
  for pool in (1, 2):
    dYd = dv(dy[pool])
    for relu in (0, 1):
      tag = 'r%dp%d' % (relu, pool)
      # ---- forward (group 0) ----
      y = new(B, H // pool, W // pool, C_)
      rn.check(lib.ra_bn_act_pool_f32(p(Ud[0]), p(Md[0]), p(Vd[0]), p(Gd[0]), p(Bd[0]), EPS, relu, pool, B, H, W, C_, p(y), st()), 'forward')
      out(y)
      err('fwd.' + tag, y, _fwd_ref(u[0], mean[0], var[0], gamma[0], beta[0], relu, pool), rel_to_max=True)
      # ---- backward per call: accumulating for every group, plain for group 0 ----
      du1, dg1, db1 = new(G, B, H, W, C_), new(G, C_), new(G, C_)
      accg, accb = torch.zeros(G, C_, device=dev), torch.zeros(G, C_, device=dev)
      for g in range(G):
        rn.check(lib.ra_bn_act_pool_bwd_acc_f32(p(Ud[g]), p(dYd[g]), p(Md[g]), p(Vd[g]), p(Gd[g]), p(Bd[g]), EPS, relu, pool, B, H, W, C_,
                                                p(ws), nbn, p(dg1[g]), p(db1[g]), p(du1[g]), p(accg[g]), p(accb[g]), st()), 'bwd acc')
      out(du1, dg1, db1)
      same('bucket %s' % tag, (accg, accb), (dg1, db1))
      rdu, rdg, rdb = _bn_bwd_ref(u[0], dy[pool][0], None, None, gamma[0], beta[0], relu, pool, EPS)
      err('du.' + tag, du1[0], rdu), err('dgamma.' + tag, dg1[0], rdg), err('dbeta.' + tag, db1[0], rdb)
      du0, dg0, db0 = new(B, H, W, C_), new(C_), new(C_)
      rn.check(lib.ra_bn_act_pool_bwd_f32(p(Ud[0]), p(dYd[0]), p(Md[0]), p(Vd[0]), p(Gd[0]), p(Bd[0]), EPS, relu, pool, B, H, W, C_, p(ws), nbn,
                                          p(dg0), p(db0), p(du0), st()), 'bwd')
      same('plain %s' % tag, (du0, dg0, db0), (du1[0], dg1[0], db1[0]))
      # ---- split: reduce | dx with this call's count, then with twice the count ----
      dgs, dbs, ag, ab, dus = new(C_), new(C_), torch.zeros(C_, device=dev), torch.zeros(C_, device=dev), new(B, H, W, C_)
      rn.check(lib.ra_bn_act_pool_bwd_reduce_f32(p(Ud[0]), p(dYd[0]), p(Md[0]), p(Vd[0]), p(Gd[0]), p(Bd[0]), EPS, relu, pool, B, H, W, C_, p(ws),
                                                 nbn, p(dgs), p(dbs), p(ag), p(ab), st()), 'reduce')
      rn.check(lib.ra_bn_act_pool_bwd_dx_f32(p(Ud[0]), p(dYd[0]), p(Md[0]), p(Vd[0]), p(Gd[0]), p(Bd[0]), p(dgs), p(dbs), 0.0, EPS, relu, pool,
                                             B, H, W, C_, p(dus), st()), 'dx')
      out(dus, dgs, dbs)
      same('split bucket %s' % tag, (ag, ab), (dgs, dbs))
      if f_split == f_bwd:
        same('split %s' % tag, (dus, dgs, dbs), (du0, dg0, db0))
      else:
        err('du.split-' + tag, dus, rdu), err('dgamma.split-' + tag, dgs, rdg), err('dbeta.split-' + tag, dbs, rdb)
      rn.check(lib.ra_bn_act_pool_bwd_dx_f32(p(Ud[0]), p(dYd[0]), p(Md[0]), p(Vd[0]), p(Gd[0]), p(Bd[0]), p(dgs), p(dbs), 2.0 * B * H * W, EPS,
                                             relu, pool, B, H, W, C_, p(dus), st()), 'dx 2n')
      out(dus)
      err('du.2n-' + tag, dus, _bn_bwd_ref(u[0], dy[pool][0], None, None, gamma[0], beta[0], relu, pool, EPS, n_total=2.0 * B * H * W)[0])
      # ---- grouped: the bits of the per-call results and a second addition to the buckets, or the refusal ----
      tabs = torch.tensor([t[g].data_ptr() for t in (Md, Vd, Gd, Bd, accg, accb) for g in range(G)], dtype=torch.int64, device=dev)
      wsg, du2, dg2, db2 = new(G * nbn), new(G, B, H, W, C_), new(G, C_), new(G, C_)
      rc = lib.ra_bn_act_pool_bwd_grouped_f32(p(Ud), p(dYd), p(tabs), G, EPS, relu, pool, B, H, W, C_, p(wsg), G * nbn, p(dg2), p(db2), p(du2), st())
      out(du2, dg2, db2, accg, accb)
      if isinstance(f_grp, int):
        if rc != f_grp or not all(bool(torch.isnan(t).all()) for t in (du2, dg2, db2)) or not torch.equal(accg, dg1):
          bad.append('grouped %s: status %d, expected %d and nothing written' % (tag, rc, f_grp))
      else:
        rn.check(rc, 'grouped')
        same('grouped %s' % tag, (du2, dg2, db2, accg, accb), (du1, dg1, db1, 2 * dg1, 2 * db1))
    # ---- bf16 storage (relu 1): the float4 kernels on bf16-exact values, or the refusal ----
    ub, dyb = Ud.bfloat16(), dYd.bfloat16()
    uf, dyf = ub.float(), dyb.float()
    yref, y3 = new(B, H // pool, W // pool, C_), torch.zeros((B, H // pool, W // pool, C_), dtype=torch.bfloat16, device=dev)
    y1 = new(B, H // pool, W // pool, C_)
    duref, dgref, dbref, agref, abref = new(G, B, H, W, C_), new(G, C_), new(G, C_), torch.zeros(G, C_, device=dev), torch.zeros(G, C_, device=dev)
    if f_fwd == 'v4':
      rn.check(lib.ra_bn_act_pool_f32(p(uf[0]), p(Md[0]), p(Vd[0]), p(Gd[0]), p(Bd[0]), EPS, 1, pool, B, H, W, C_, p(yref), st()), 'fwd ref')
    if f_grp == 'v4':
      tabs = torch.tensor([t[g].data_ptr() for t in (Md, Vd, Gd, Bd, agref, abref) for g in range(G)], dtype=torch.int64, device=dev)
      rn.check(lib.ra_bn_act_pool_bwd_grouped_f32(p(uf), p(dyf), p(tabs), G, EPS, 1, pool, B, H, W, C_, p(wsg), G * nbn, p(dgref), p(dbref),
                                                  p(duref), st()), 'grouped ref')
    for flags, dyx in ((1, dyf), (3, dyb)):
      yx = y3 if flags & 2 else y1
      rc = lib.ra_bn_act_pool_bf16_f32(p(ub[0]), p(Md[0]), p(Vd[0]), p(Gd[0]), p(Bd[0]), EPS, 1, pool, B, H, W, C_, p(yx), flags, st())
      du3, dg3, db3, ag3, ab3 = torch.zeros_like(ub), new(G, C_), new(G, C_), torch.zeros(G, C_, device=dev), torch.zeros(G, C_, device=dev)
      tabs = torch.tensor([t[g].data_ptr() for t in (Md, Vd, Gd, Bd, ag3, ab3) for g in range(G)], dtype=torch.int64, device=dev)
      rcg = lib.ra_bn_act_pool_bwd_grouped_bf16_f32(p(ub), p(dyx), p(tabs), G, EPS, 1, pool, B, H, W, C_, p(wsg), G * nbn, p(dg3), p(db3), p(du3),
                                                    flags, st())
      du4, dg4, db4, ag4, ab4 = torch.zeros_like(ub[0]), new(C_), new(C_), torch.zeros(C_, device=dev), torch.zeros(C_, device=dev)
      rcc = lib.ra_bn_act_pool_bwd_acc_bf16_f32(p(ub[0]), p(dyx[0]), p(Md[0]), p(Vd[0]), p(Gd[0]), p(Bd[0]), EPS, 1, pool, B, H, W, C_, p(ws), nbn,
                                                p(dg4), p(db4), p(du4), p(ag4), p(ab4), flags, st())
      out(yx, du3, dg3, db3, ag3, ab3, du4, dg4, db4, ag4, ab4)
      tag = 'flags %d pool %d' % (flags, pool)
      if f_fwd == 'v4':
        rn.check(rc, 'fwd bf16'), rn.check(rcg, 'grouped bf16'), rn.check(rcc, 'acc bf16')
        same('forward ' + tag, (yx,), (yref.bfloat16() if flags & 2 else yref,))
        same('grouped ' + tag, (du3, dg3, db3, ag3, ab3), (duref.bfloat16(), dgref, dbref, agref, abref))
        same('per call ' + tag, (du4, dg4, db4, ag4, ab4), (duref[0].bfloat16(), dgref[0], dbref[0], agref[0], abref[0]))
      elif (rc, rcg, rcc) != (E_SHAPE,) * 3 or bool(du3.any()) or bool(du4.any()) or bool(ag3.any()) or bool(ag4.any()) or not (
          bool(torch.isnan(y1).all()) and not bool(y3.any()) and bool(torch.isnan(dg3).all()) and bool(torch.isnan(dg4).all())):
        bad.append('%s: status %d / %d / %d, expected %d and nothing written' % (tag, rc, rcg, rcc, E_SHAPE))
  return sha.hexdigest(), errs, bad


def parse_line(line):
  """A runner line -> (name, sha256, [(err, bar), ...]), or None for any other line."""
  f = line.split()
  if len(f) < 4 or f[0] != 'case':
    return None
  return f[1], f[3], [tuple(float(v) for v in q.split(':')[-2:]) for q in f[4:]]


def digest_text(line):
  """A runner line as tools/bn_digest.py compares it between builds: without the forms (a build from before ra_bn_form prints '-')."""
  f = line.split()
  return ' '.join(f[:2] + f[3:])


def main():
  import argparse
  ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
  ap.add_argument('--lib', help='the librecattend.so to run (default: the tree\'s own)')
  ap.add_argument('--verbose', action='store_true', help='name each error (what:err:bar)')
  args = ap.parse_args()
  import ra_native as rn
  if args.lib:
    rn.LIB_PATH = os.path.abspath(args.lib)
    if not hasattr(C.CDLL(rn.LIB_PATH), 'ra_bn_form'):  # a build from before the query: its forms print as '-'
      del rn.SIGNATURES['ra_bn_form']
  if not torch.cuda.is_available():
    raise SystemExit('bn_form_cases: needs an MI355X')
  torch.set_num_threads(1)  # the float64 references are summed in one order
  dev = torch.device('cuda')
  lib = rn.lib()
  broken = 0
  for case in CASES:
    ties = pool_ties(inputs(case)[0])
    forms = reported_forms(lib, case) if 'ra_bn_form' in rn.SIGNATURES else None
    sha, errs, bad = run_case(lib, rn, case, dev)
    print('case %s %s %s %s' % (case['name'], '/'.join(map(str, forms)) if forms else '-', sha,
                                ' '.join(('%s:%.3e:%g' if args.verbose else '%.0s%.3e:%g') % e for e in errs)), flush=True)
    for b in bad + (['%d pool windows with a tied maximum' % ties] if ties else []):
      print('BROKEN %s: %s' % (case['name'], b), flush=True)
      broken += 1
  return 1 if broken else 0


if __name__ == '__main__':
  sys.exit(main())
