"""The training step's controller kernels (csrc/ra_ctrl_train.hip) over their dimension space: one table of cases, one reference.

ctrl_fwd_kernel / ctrl_bwd_kernel are one 1024-thread workgroup per image whose LDS carve, GEMV partitioning and wave loops all
follow from (G, Cf, hid, iters, n_g, n_c, mlp).  CASES walks those dimensions at the smallest points where each choice can go
wrong; reference() restates full_model.py:668-689 (glimpse read-out, LSTM, glimpse MLP with a softmax over the map, controller
MLP) in torch on the CPU, in float64 or float32, and returns through autograd everything the kernels put out:

  h_last, co, the saved rows in the kernels' own layout, save_c, and for each of the four combinations of upstream gradients
  (d h_last and d co each present or absent) d feat, the pre-activation gradients dpre / dlog / dzg[l] / dzc[l] and every
  parameter gradient.  (The pre-activation gradients are taken with autograd.grad on the pre-activation tensors themselves:
  what retain_grad would leave in their .grad, for four backward passes over one graph.)

param_grads_from_rows() forms the parameter gradients as ra_train._CtrlStepBuffers.__call__ does, A^T B over the saved rows and
the pre-activation gradients at the same offsets (the glimpse MLP's first layer one row ahead), in float64 NumPy.

forward_scores() / grad_scores() / param_scores() are the one table of bars; tests/test_ctrl_train.py asserts on the CPU that the
float32 run of the reference sits CONDITIONING inside each, tests/test_ctrl_train_gpu.py asserts the kernels against them.

  python tests/ctrl_train_cases.py            the kernels' largest error per row and quantity (needs an MI355X)
  python tests/ctrl_train_cases.py --search   seeds per row under which the three input conditions hold (host only)
"""
import collections
import functools
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, 'rec-attend-public_amd'), os.path.join(ROOT, 'oracle')):
  if _p not in sys.path:
    sys.path.insert(0, _p)

NOUT = 9
# ---- bars: the controller's own (ctrl_form_cases.errors) and the tightest gradient bar test_controller_fn_unit_vs_library holds
TOL_H = 5e-5      # h_last, relative to the image's |ref| max
TOL_CO = 5e-5     # co, absolute
TOL_MAP = 1e-5    # glimpse maps, absolute
TOL_SAVED = 5e-5  # every other saved field, relative to the image's |ref| max of that field
TOL_GRAD = 2e-5   # every gradient, relative to the image's (parameter gradients: the tensor's) own |ref| max; no floor
CONDITIONING = 8.0  # attn_geometry_cases' factor: the float32 CPU run of the reference sits this far inside every bar
RELU_MARGIN = 1e-4  # every ReLU pre-activation of the float64 run is at least this far from its kink
MAP_PEAK = 3.0      # the largest weight of every non-initial glimpse map is at least MAP_PEAK / G

# the largest G ra_ctrl_train_supported_n accepts at Cf = 64, hid = 256 (two controller-MLP layers or one): the backward's
# 64 + 6 hid + (Cf + hid) + G + max(hid, G, mlp) + max(hid, mlp) + 2 G Cf floats against 160 KiB.  tests/test_ctrl_train.py
# finds it again by host query and fails if the two differ.
G_LDS_BOUND = 296

Case = collections.namedtuple('Case', 'name G Cf hid iters n_g n_c mlp B seed gain what')

# gain: what the last glimpse layer's weights are multiplied by, so that the map is not uniform
# seed: found by --search; the three conditions on the inputs hold under it (asserted by tests/test_ctrl_train.py)
CASES = [
    Case('run128', 16, 64, 256, 5, 2, 1, 0, 3, 3, 8.0, 'the run scripts\' point at 128 x 128'),
    Case('kitti', 56, 64, 256, 5, 2, 1, 0, 2, 2, 8.0, 'KITTI\'s 4 x 14 map: G no multiple of 16, the wave-per-row loops end on a ragged pass'),
    Case('cfg2', 256, 64, 256, 5, 2, 1, 0, 2, 0, 8.0, 'cfg2\'s 16 x 16 map'),
    Case('lds-bound', G_LDS_BOUND, 64, 256, 5, 2, 1, 0, 1, 0, 8.0, 'the largest G the support query accepts: one 159 KB workgroup'),
    Case('hid8', 16, 64, 8, 3, 2, 1, 0, 3, 7, 24.0, 'hid < 16: the read-out\'s partial sums are the larger user of the scratch'),
    Case('smallest', 8, 4, 4, 2, 1, 1, 0, 2, 11, 40.0, 'hid < 16 at the smallest of everything: 1024 partial sums against 256 GEMV floats'),
    Case('g-mlp-bound', 64, 8, 16, 3, 2, 2, 64, 2, 1, 24.0, 'G = 4 hid and mlp = 4 hid, both at their bound'),
    Case('cf100', 12, 100, 32, 3, 3, 2, 20, 3, 1, 16.0, 'Cf above 64 and no multiple of it: 1024 / Cf leaves idle threads in the read-out'),
    Case('cf1024', 4, 1024, 16, 2, 2, 1, 0, 2, 5, 40.0, 'one read-out part'),
    Case('iters1', 16, 64, 32, 1, 2, 2, 48, 2, 0, 16.0, 'iters = 1: the glimpse MLP never runs; dlog, dzg and the saved z are exactly zero'),
    Case('ng1', 16, 32, 16, 3, 1, 4, 64, 2, 1, 40.0, 'n_g = 1: the gemv_rows(..., dh, accumulate) branch, with mlp > hid'),
    Case('depth4', 16, 32, 32, 4, 4, 4, 4, 2, 0, 24.0, 'both MLPs at kMaxL; mlp = 4'),
]
CASE_OF = {c.name: c for c in CASES}
COMBOS = [(True, True), (True, False), (False, True), (False, False)]  # (d h_last given, d co given)


def combo_id(combo):
  return '%s-%s' % ('dh' if combo[0] else 'none', 'dco' if combo[1] else 'none')


def save_floats(c):
  """Floats of one (image, iteration)'s saved row: xh | act | c | z | gm."""
  return (c.Cf + c.hid) + 4 * c.hid + c.hid + (c.n_g - 1) * c.hid + c.G


def fields(c):
  """name -> slice of a saved row, in the kernels' order (ra_ctrl_train.hip, save_floats)."""
  out, at = collections.OrderedDict(), 0
  for name, n in (('glimpse', c.Cf), ('h_prev', c.hid), ('gate_i', c.hid), ('gate_f', c.hid), ('gate_o', c.hid), ('gate_u', c.hid), ('c', c.hid)):
    out[name] = slice(at, at + n)
    at += n
  for l in range(c.n_g - 1):
    out['z%d' % l] = slice(at, at + c.hid)
    at += c.hid
  out['map'] = slice(at, at + c.G)
  assert at + c.G == save_floats(c)
  return out


def inputs(c):
  """The case's float32 inputs: two feature maps (ReLU of a normal draw, as ctrl_form_cases draws them), weights a normal draw
  times min(0.15, 1.5 / sqrt(K)) with the last glimpse layer times c.gain, biases a normal draw times 0.1, the upstream gradients."""
  rng = np.random.RandomState(1000 * [k.name for k in CASES].index(c.name) + c.seed)
  f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
  w = lambda K, N: f32(rng.randn(K, N) * min(0.15, 1.5 / np.sqrt(K)))
  b = lambda N: f32(rng.randn(N) * 0.1)
  x = {'feat': f32(np.maximum(rng.randn(c.B, c.G, c.Cf), 0)), 'feat2': f32(np.maximum(rng.randn(c.B, c.G, c.Cf), 0))}
  x['Wg'], x['bg'] = w(c.Cf + c.hid, 4 * c.hid), b(4 * c.hid)
  gdims = [c.hid] * c.n_g + [c.G]
  x['gW'] = [w(gdims[l], gdims[l + 1]) for l in range(c.n_g)]
  x['gW'][-1] = f32(x['gW'][-1] * c.gain)
  x['gb'] = [b(gdims[l + 1]) for l in range(c.n_g)]
  cdims = [c.hid] + [c.mlp] * (c.n_c - 1) + [NOUT]
  x['cW'] = [w(cdims[l], cdims[l + 1]) for l in range(c.n_c)]
  x['cb'] = [b(cdims[l + 1]) for l in range(c.n_c)]
  x['dh'], x['dco'] = f32(rng.randn(c.B, c.hid)), f32(rng.randn(c.B, NOUT))
  return x


def _reference(c, x, dtype):
  T = lambda a: torch.from_numpy(np.asarray(a)).to(dtype)
  leaf = lambda a: T(a).requires_grad_(True)
  feat, Wg, bg = leaf(x['feat']), leaf(x['Wg']), leaf(x['bg'])
  gW, gb, cW, cb = [[leaf(a) for a in x[k]] for k in ('gW', 'gb', 'cW', 'cb')]
  B, G, Cf, hid = c.B, c.G, c.Cf, c.hid
  h = cst = torch.zeros(B, hid, dtype=dtype)
  gm = torch.full((B, G), 1.0 / G, dtype=dtype)
  rows, pres, logs, zgs, relu_pre, peaks = [], [], [], [[] for _ in range(c.n_g - 1)], [], []
  for it in range(c.iters):
    glimpse = (feat * gm[:, :, None]).sum(dim=1)  # full_model.py:680
    xh = torch.cat([glimpse, h], dim=1)
    pre = xh @ Wg + bg
    pres.append(pre)
    gi, gf, go = [torch.sigmoid(pre[:, k * hid:(k + 1) * hid]) for k in range(3)]
    u = torch.tanh(pre[:, 3 * hid:])
    cst = gf * cst + gi * u  # nnlib.py:641-646
    h = go * torch.tanh(cst)
    zs, gm_read = [], gm
    if it < c.iters - 1:
      z = h
      for l in range(c.n_g - 1):
        zp = z @ gW[l] + gb[l]
        zgs[l].append(zp)
        relu_pre.append(zp)
        z = torch.relu(zp)
        zs.append(z)
      lg = z @ gW[-1] + gb[-1]
      logs.append(lg)
      gm = torch.softmax(lg, dim=1)
      peaks.append(gm.max(dim=1)[0] * G)
    else:  # the last iteration's map is never read (full_model.py:687): the kernels skip its glimpse MLP and save zeros
      zs = [torch.zeros(B, hid, dtype=dtype)] * (c.n_g - 1)
    rows.append(torch.cat([xh, gi, gf, go, u, cst] + zs + [gm_read], dim=1))
  z, zcs, hidden_c = h, [], []
  for l in range(c.n_c - 1):
    zp = z @ cW[l] + cb[l]
    zcs.append(zp)
    relu_pre.append(zp)
    z = torch.relu(zp)
    hidden_c.append(z)
  co = z @ cW[-1] + cb[-1]
  n64 = lambda t: t.detach().to(torch.float64).numpy()
  out = {'h_last': n64(h), 'co': n64(co), 'save': n64(torch.stack(rows, dim=1)),
         'save_c': n64(torch.cat(hidden_c, dim=1)) if hidden_c else np.zeros((B, 0)),
         'relu_min': min([float(p.detach().abs().min()) for p in relu_pre] or [np.inf]),
         'map_peak': min([float(p.detach().min()) for p in peaks] or [np.inf]), 'grads': {}}
  assert out['save'].shape == (B, c.iters, save_floats(c))
  wrt = [feat, Wg, bg] + gW + gb + cW + cb + pres + logs + [t for l in zgs for t in l] + zcs
  for combo in COMBOS:
    if combo == (False, False):
      got = [None] * len(wrt)
    else:
      loss = (h * T(x['dh'])).sum() * float(combo[0]) + (co * T(x['dco'])).sum() * float(combo[1])
      got = torch.autograd.grad(loss, wrt, retain_graph=True, allow_unused=True)
    got = collections.deque(np.zeros(tuple(t.shape)) if g is None else n64(g) for t, g in zip(wrt, got))
    take = lambda n: [got.popleft() for _ in range(n)]
    g = {'dfeat': take(1)[0]}
    gWg, gbg = take(2)
    P = {}
    for j, k in enumerate('ifou'):
      cols = slice(j * hid, (j + 1) * hid)
      P['ctrl_lstm_w_x' + k], P['ctrl_lstm_w_h' + k], P['ctrl_lstm_b_' + k] = gWg[:Cf, cols], gWg[Cf:, cols], gbg[cols]
    for name, n in (('glimpse_mlp_w_%d', c.n_g), ('glimpse_mlp_b_%d', c.n_g), ('ctrl_mlp_w_%d', c.n_c), ('ctrl_mlp_b_%d', c.n_c)):
      for l, a in enumerate(take(n)):
        P[name % l] = a
    g['params'] = P
    g['dpre'] = np.stack(take(c.iters), axis=1)
    zero_it = lambda n: [np.zeros((B, n))]  # the last iteration
    g['dlog'] = np.stack(take(c.iters - 1) + zero_it(G), axis=1)
    g['dzg'] = np.stack([np.stack(take(c.iters - 1) + zero_it(hid), axis=1) for _ in range(c.n_g - 1)], axis=0) if c.n_g > 1 else \
        np.zeros((0, B, c.iters, hid))
    g['dzc'] = np.stack(take(c.n_c - 1), axis=0) if c.n_c > 1 else np.zeros((0, B, max(c.mlp, 1)))
    assert not got
    out['grads'][combo] = g
  return out


@functools.lru_cache(maxsize=None)
def reference(name, dtype='float64'):
  """The case's reference (see the module's docstring), computed once per process and shared: callers leave it unchanged."""
  c = CASE_OF[name]
  return _reference(c, inputs(c), getattr(torch, dtype))


def param_grads_from_rows(c, h_last, save, save_c, g, dco):
  """Every parameter gradient as (layer input)^T (pre-activation gradient) over the saved rows, at the offsets of
  ra_train._CtrlStepBuffers.__call__, in float64.  g: dpre, dlog, dzg [n_g - 1, B, iters, hid], dzc [n_c - 1, B, mlp]; dco [B, 9]."""
  f8 = lambda a: np.asarray(a, dtype=np.float64)
  Cf, hid, it, n_g, n_c, mlp = c.Cf, c.hid, c.iters, c.n_g, c.n_c, c.mlp
  save, n = f8(save), c.B * c.iters
  rows, D = save.reshape(n, -1), f8(g['dpre']).reshape(n, 4 * hid)
  gWg = rows[:, :Cf + hid].T @ D
  P = {}
  for j, k in enumerate('ifou'):
    cols = slice(j * hid, (j + 1) * hid)
    P['ctrl_lstm_w_x' + k], P['ctrl_lstm_w_h' + k], P['ctrl_lstm_b_' + k] = gWg[:Cf, cols], gWg[Cf:, cols], D[:, cols].sum(axis=0)
  H0 = save[:, 1:, Cf:Cf + hid].reshape(-1, hid)  # h after the LSTM of (b, it) = the h half of iteration it + 1's LSTM input
  for l in range(n_g):
    A = H0 if l == 0 else rows[:, Cf + 6 * hid + (l - 1) * hid:Cf + 6 * hid + l * hid]
    Bm = f8(g['dlog']) if l == n_g - 1 else f8(g['dzg'][l])
    Bm = Bm[:, :-1].reshape(-1, Bm.shape[-1]) if l == 0 else Bm.reshape(n, -1)
    P['glimpse_mlp_w_%d' % l], P['glimpse_mlp_b_%d' % l] = A.T @ Bm, Bm.sum(axis=0)
  for l in range(n_c):
    A = f8(h_last) if l == 0 else f8(save_c)[:, (l - 1) * mlp:l * mlp]
    Bm = f8(dco) if l == n_c - 1 else f8(g['dzc'][l])
    P['ctrl_mlp_w_%d' % l], P['ctrl_mlp_b_%d' % l] = A.T @ Bm, Bm.sum(axis=0)
  return P


# ---- scoring: [(what, err, bar), ...]; a case passes where every err < bar

def _per_image(got, ref, baxis, relative):
  """The largest error over the images, each image's own: |got - ref| max, over that image's |ref| max where relative.  An image
  whose reference is identically zero must be exactly zero (inf otherwise): there is no floor to hide behind."""
  got, ref = [np.moveaxis(np.asarray(a, dtype=np.float64), baxis, 0).reshape(ref.shape[baxis], -1) for a in (got, ref)]
  assert got.shape == ref.shape, (got.shape, ref.shape)
  if got.shape[1] == 0:
    return 0.0
  e, m = np.abs(got - ref).max(axis=1), np.abs(ref).max(axis=1)
  if not relative:
    return float(e.max())
  return float(np.where(m > 0, e / np.where(m > 0, m, 1.0), np.where(e == 0, 0.0, np.inf)).max())


def forward_scores(c, ref, got):
  out = [('h_last', _per_image(got['h_last'], ref['h_last'], 0, True), TOL_H), ('co', _per_image(got['co'], ref['co'], 0, False), TOL_CO)]
  for name, sl in fields(c).items():
    a, b = np.asarray(got['save'])[:, :, sl], ref['save'][:, :, sl]
    out.append(('save.' + name, _per_image(a, b, 0, name != 'map'), TOL_MAP if name == 'map' else TOL_SAVED))
  for l in range(c.n_c - 1):
    sl = slice(l * c.mlp, (l + 1) * c.mlp)
    out.append(('save_c.z%d' % l, _per_image(np.asarray(got['save_c'])[:, sl], ref['save_c'][:, sl], 0, True), TOL_SAVED))
  return out


def grad_scores(c, refg, gotg, combo):
  """d feat and the pre-activation gradients of one combination of upstream gradients; dzc only where d co is given (the
  kernel leaves it alone otherwise)."""
  out = [(k, _per_image(gotg[k], refg[k], 0, True), TOL_GRAD) for k in ('dfeat', 'dpre', 'dlog')]
  out += [('dzg%d' % l, _per_image(gotg['dzg'][l], refg['dzg'][l], 0, True), TOL_GRAD) for l in range(c.n_g - 1)]
  if combo[1]:
    out += [('dzc%d' % l, _per_image(gotg['dzc'][l], refg['dzc'][l], 0, True), TOL_GRAD) for l in range(c.n_c - 1)]
  return out


def param_scores(refP, gotP):
  assert sorted(refP) == sorted(gotP)
  return [('d ' + k, _per_image(gotP[k][None], refP[k][None], 0, True), TOL_GRAD) for k in sorted(refP)]


def all_scores(c, ref, got):
  """Every score of a case: forward, then per combination the gradients and the parameter gradients formed from got's OWN rows."""
  out = forward_scores(c, ref, got)
  x = inputs(c)
  for combo in COMBOS:
    g, rg = got['grads'][combo], ref['grads'][combo]
    tag = combo_id(combo) + ':'
    out += [(tag + w, e, bar) for w, e, bar in grad_scores(c, rg, g, combo)]
    gz = dict(g, dzc=g['dzc'] if combo[1] else np.zeros_like(rg['dzc']))  # rows the kernel left to the caller: zeroed, as begin_step does
    P = param_grads_from_rows(c, got['h_last'], got['save'], got['save_c'], gz, x['dco'] if combo[1] else np.zeros_like(x['dco']))
    out += [(tag + w, e, bar) for w, e, bar in param_scores(rg['params'], P)]
  return out


def conditions(c, seed=None):
  """(smallest |ReLU pre-activation| of the float64 run, smallest G * max of a non-initial map, the float32 CPU run's largest
  err / bar over all_scores) under the case's seed or another."""
  if seed is None:
    r64, r32 = reference(c.name), reference(c.name, 'float32')
  else:
    c = c._replace(seed=seed)
    r64, r32 = _reference(c, inputs(c), torch.float64), _reference(c, inputs(c), torch.float32)
  worst = max((e / bar, w) for w, e, bar in all_scores(c, r64, r32))
  return r64['relu_min'], r64['map_peak'], worst


def conditions_hold(relu_min, map_peak, worst):
  return relu_min >= RELU_MARGIN and map_peak >= MAP_PEAK and worst[0] * CONDITIONING <= 1.0


# ---- the kernels through the C ABI (needs an MI355X)

GUARD = 64             # sentinel floats either side of every output (test_conv_forms_gpu.Guarded's pattern)
SENTINEL = 0x4b3c2d1e  # a float32 bit pattern no kernel here computes


class Guarded(object):
  """An output view inside a buffer of sentinel words.  fill = None: NaN, and result() insists that every element was written."""

  def __init__(self, shape, dev, fill=None):
    n = int(np.prod(shape))
    self.buf = torch.empty(n + 2 * GUARD, dtype=torch.float32, device=dev)
    self.buf.view(torch.int32).fill_(SENTINEL)
    self.view = self.buf[GUARD:GUARD + n].view(shape)
    self.view.fill_(float('nan') if fill is None else fill)
    assert self.view.data_ptr() % 16 == 0
    self.n, self.must_be_written = n, fill is None

  def result(self, what):
    torch.cuda.synchronize()
    bits = self.buf.view(torch.int32).cpu().numpy()
    lo, hi = bits[:GUARD], bits[GUARD + self.n:]
    assert (lo == SENTINEL).all() and (hi == SENTINEL).all(), '%s: wrote outside its output: %d words before, %d after' % (
        what, int((lo != SENTINEL).sum()), int((hi != SENTINEL).sum()))
    y = self.view.cpu().numpy()
    if self.must_be_written:
      holes = np.argwhere(np.isnan(y))
      assert len(holes) == 0, '%s: %d output elements never written, first %s' % (what, len(holes), tuple(int(v) for v in holes[0]))
    return y


def device_inputs(c, dev):
  x = inputs(c)
  t = lambda a: torch.from_numpy(a).to(dev)
  return {k: [t(a) for a in v] if isinstance(v, list) else t(v) for k, v in x.items()}


def _arr(ts):
  import ctypes as C
  return (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def forward_buffers(c, dev):
  return {'h_last': Guarded((c.B, c.hid), dev), 'co': Guarded((c.B, NOUT), dev), 'save': Guarded((c.B, c.iters, save_floats(c)), dev),
          'save_c': Guarded((c.B, (c.n_c - 1) * c.mlp), dev) if c.n_c > 1 else None}


def launch_forward(c, xd, feat, out):
  import ra_native as rn
  rn.check(rn.lib().ra_ctrl_train_fwd_n_f32(c.B, c.G, c.Cf, c.hid, c.iters, NOUT, c.n_g, c.n_c, c.mlp, rn.ptr(feat), rn.ptr(xd['Wg']),
                                            rn.ptr(xd['bg']), _arr(xd['gW']), _arr(xd['gb']), _arr(xd['cW']), _arr(xd['cb']),
                                            rn.ptr(out['h_last'].view), rn.ptr(out['co'].view), rn.ptr(out['save'].view),
                                            rn.ptr(out['save_c'].view) if c.n_c > 1 else None, rn.stream_ptr()), 'ra_ctrl_train_fwd_n_f32')


def forward_results(c, out, what):
  r = {k: out[k].result('%s %s' % (what, k)) for k in ('h_last', 'co', 'save')}
  r['save_c'] = out['save_c'].result(what + ' save_c') if c.n_c > 1 else np.zeros((c.B, 0), np.float32)
  return r


DZC_FILL = 123.0  # what the caller leaves in the dzc rows before a launch without d co


def launch_backward(c, xd, fwd, combo, dev, gap=0):
  """One backward launch over the forward's buffers fwd -> dict of numpy results.  gap > 0: the layers of dzg / dzc lie gap floats
  further apart than one layer (the stacked step's 'all' view); the floats between them must come back as sentinels."""
  import ra_native as rn
  B, G, hid, it = c.B, c.G, c.hid, c.iters
  o = {'dfeat': Guarded((B, G, c.Cf), dev), 'dpre': Guarded((B, it, 4 * hid), dev), 'dlog': Guarded((B, it, G), dev)}
  Lg, Lc, ng, nc = B * it * hid, B * c.mlp, c.n_g - 1, c.n_c - 1
  sg, sc = Lg + gap, Lc + gap
  assert gap % 4 == 0
  dzg = Guarded((ng * sg,), dev) if ng else None
  dzc = Guarded((nc * sc,), dev, fill=None if combo[1] else DZC_FILL) if nc else None
  for t, L, s, n in ((dzg, Lg, sg, ng), (dzc, Lc, sc, nc)):
    for l in range(n):
      t.view[l * s + L:(l + 1) * s].view(torch.int32).fill_(SENTINEL)
  rn.check(rn.lib().ra_ctrl_train_bwd_n_f32(B, G, c.Cf, hid, it, NOUT, c.n_g, c.n_c, c.mlp, rn.ptr(xd['feat']), rn.ptr(xd['Wg']), _arr(xd['gW']),
                                            _arr(xd['cW']), rn.ptr(fwd['save'].view), rn.ptr(fwd['save_c'].view) if nc else None,
                                            rn.ptr(xd['dh']) if combo[0] else None, rn.ptr(xd['dco']) if combo[1] else None,
                                            rn.ptr(o['dfeat'].view), rn.ptr(o['dpre'].view), rn.ptr(o['dlog'].view),
                                            rn.ptr(dzg.view) if ng else None, sg, rn.ptr(dzc.view) if nc else None, sc, rn.stream_ptr()),
           'ra_ctrl_train_bwd_n_f32')
  what = '%s backward %s' % (c.name, combo_id(combo))
  r = {k: v.result('%s %s' % (what, k)) for k, v in o.items()}
  for key, t, L, s, n, shape in (('dzg', dzg, Lg, sg, ng, (B, it, hid)), ('dzc', dzc, Lc, sc, nc, (B, c.mlp))):
    if not n:
      r[key] = np.zeros((0,) + shape, np.float32)
      continue
    torch.cuda.synchronize()
    bits = t.view.view(torch.int32).cpu().numpy().reshape(n, s)
    assert (bits[:, L:] == SENTINEL).all(), '%s %s: wrote between its layers' % (what, key)
    flat = t.view.view(n, s)[:, :L].clone()
    t.view.view(n, s)[:, L:] = 0.0  # the gaps are checked: result() looks for holes in the layers and at the outer guards
    t.result('%s %s' % (what, key))
    r[key] = flat.cpu().numpy().reshape((n,) + shape)
  return r


def run_kernels(c, dev):
  """Forward and the four backward launches of a case -> a dict shaped like reference()'s."""
  xd = device_inputs(c, dev)
  out = forward_buffers(c, dev)
  launch_forward(c, xd, xd['feat'], out)
  got = forward_results(c, out, c.name + ' forward')
  got['grads'] = {combo: launch_backward(c, xd, out, combo, dev) for combo in COMBOS}
  return got


def worst_by_quantity(scores):
  """all_scores' list -> [(what, err, bar)] with the combinations folded: the largest err per quantity."""
  out = collections.OrderedDict()
  for w, e, bar in scores:
    w = w.split(':')[-1]
    out[w] = (max(e, out[w][0]) if w in out else e, bar)
  return [(w, e, bar) for w, (e, bar) in out.items()]


def main():
  import argparse
  ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
  ap.add_argument('--search', action='store_true', help='print, per row, the first seed under which the input conditions hold')
  args = ap.parse_args()
  if args.search:
    for c in CASES:
      for seed in range(200):
        cond = conditions(c, seed)
        if conditions_hold(*cond):
          break
      print('%-12s seed %3d  min |relu pre| %.2e  G max(map) %.2f  float32 run %.3f of the bar at %s' % ((c.name, seed) + cond[:2] + cond[2]), flush=True)
    return
  if not torch.cuda.is_available():
    raise SystemExit('ctrl_train_cases: needs an MI355X')
  dev = torch.device('cuda')
  for c in CASES:
    scores = all_scores(c, reference(c.name), run_kernels(c, dev))
    print('case %-12s (G %d Cf %d hid %d iters %d n_g %d n_c %d mlp %d B %d) worst %.3f of its bar' % (
        (c.name,) + tuple(c[1:9]) + (max(e / bar for _, e, bar in scores),)))
    for w, e, bar in worst_by_quantity(scores):
      print('  %-22s %.3e  bar %g' % (w, e, bar), flush=True)


if __name__ == '__main__':
  main()
