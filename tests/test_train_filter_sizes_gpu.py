"""Training with filter sizes 1, 5 and 7 on the MI355X (model_opt['train_any_filter']; nnlib.py:131-257, :260-404): the k x k
filter-gradient kernel (csrc/ra_wgrad_kxk.hip) against float64 sums, ConvBNActPool and the nnlib closures against float64 torch
autograd, then the whole training step of full_model / box_model with mixed sizes against ra_oracle_torch, two optimizer steps
and the command lines.  ra_oracle_torch.deconv_same crops a stride-2 transposed conv at 0, which is right for size 3 alone: these
tests put train_filter_cases.deconv_ref in its place (test_train_filter_sizes.py pins it to ra_oracle.conv2d_transpose)."""
import numpy as np
import pytest
import torch

import ra_native as rn
import ra_ops as ops
import ra_oracle_torch as ort
import ra_train
import train_filter_cases as tfc
from wgrad_form_cases import F32_BAR, MAPS, _rel as _rel_t

pytestmark = pytest.mark.gpu

SHAPES = [(2, 9, 33), (1, 8, 32), (1, 5, 6), (3, 20, 40)]  # ragged 2 x 2 tiles; one tile; smaller than the 7-tap halo; several tiles a workgroup
PAIRS = [(4, 8), (8, 1), (12, 8), (20, 16), (16, 48), (32, 128), (40, 96)]
_FORMS = {}  # (kf) -> the NT values the cases reached, checked by test_every_launch_form_was_reached


def _run(kf, x, du, ups=0, acc=None, g0=None):
  """One launch on NaN-filled workspace and outputs.  acc: (chan_map list or None, cin_w, transposed) -> onto g0 = (gw, gb)."""
  lib = rn.lib()
  B, Hs, Ws, cin = x.shape
  H, W, cout = du.shape[1:]
  nws = lib.ra_convkxk_wgrad_workspace_floats(kf, cin, cout, B, H, W)
  assert nws > 0
  ws = torch.full((nws,), float('nan'), device=x.device)
  if acc is None:
    ow, ob = torch.full((kf, kf, cin, cout), float('nan'), device=x.device), torch.full((cout,), float('nan'), device=x.device)
    rn.check(lib.ra_convkxk_wgrad_f32(rn.ptr(x), cin, B, Hs, Ws, ups, rn.ptr(du), cout, kf, rn.ptr(ws), nws, rn.ptr(ow), rn.ptr(ob),
                                      rn.stream_ptr()), 'ra_convkxk_wgrad_f32')
  else:
    cmap, cin_w, tr = acc
    ow, ob = g0[0].clone(), g0[1].clone()
    cm = torch.tensor(cmap, dtype=torch.int32, device=x.device) if cmap is not None else None
    rn.check(lib.ra_convkxk_wgrad_acc_f32(rn.ptr(x), cin, B, Hs, Ws, ups, rn.ptr(du), cout, kf, rn.ptr(ws), nws, rn.ptr(cm), cin_w, tr,
                                          rn.ptr(ow), rn.ptr(ob), rn.stream_ptr()), 'ra_convkxk_wgrad_acc_f32')
  torch.cuda.synchronize()
  _FORMS.setdefault(kf, set()).add(ops.wgrad_kxk_plan(kf, cin, cout, B, H, W)['nt'])
  return ow, ob


def _draw(seed, B, Hs, Ws, cin, cout, ups, dev):
  """x ~ N(0, 1), du ~ N(0.5, 1).  The bar is an error relative to max |ref|, and with ONE output channel max |db| is a single
  sum: of zero-mean values it cancels to anything (a first run drew 1 224 of them summing to 0.3 % of their size, and a float32
  sum exact to 1e-7 of the terms read 1.3e-4 against it).  A mean keeps that sum, like every other, at the size of its terms."""
  rng = np.random.RandomState(seed)
  up = 1 + ups
  return (torch.from_numpy(rng.randn(B, Hs, Ws, cin).astype(np.float32)).to(dev),
          torch.from_numpy((rng.randn(B, Hs * up, Ws * up, cout) + 0.5).astype(np.float32)).to(dev), rng)


@pytest.mark.parametrize('kf', tfc.SIZES)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_wgrad_kxk_vs_float64(cuda, kf, shape):
  B, H, W = shape
  for cin, cout in PAIRS:
    x, du, _ = _draw(1000 * cin + 10 * cout + H + kf, B, H, W, cin, cout, 0, cuda)
    ow, ob = _run(kf, x, du)
    assert not torch.isnan(ow).any() and not torch.isnan(ob).any(), (cin, cout)
    rw, rb = tfc.wgrad_ref(x, du, kf)
    ew, eb = _rel_t(ow, rw), _rel_t(ob, rb)
    print('kf %d %s %dx%d: dw %.2e db %.2e' % (kf, shape, cin, cout, ew, eb))
    assert ew < F32_BAR and eb < F32_BAR, (cin, cout, ew, eb)
    ow2, ob2 = _run(kf, x, du)  # fixed summation order, no atomics: the same bytes
    assert torch.equal(ow, ow2) and torch.equal(ob, ob2), (cin, cout)


@pytest.mark.parametrize('kf', tfc.SIZES)
@pytest.mark.parametrize('Hs,Ws', [(3, 5), (9, 17)])
def test_wgrad_kxk_upsample_vs_autograd_of_the_transposed_conv(cuda, kf, Hs, Ws):
  for cin, cout in [(8, 8), (16, 16), (32, 16), (8, 1), (20, 48)]:
    x, du, _ = _draw(77 * cin + cout + Hs + kf, 2, Hs, Ws, cin, cout, 1, cuda)
    ow, ob = _run(kf, x, du, ups=1)
    assert not torch.isnan(ow).any() and not torch.isnan(ob).any()
    rw, rb = tfc.wgrad_ref_ups(x.cpu(), du.cpu(), kf)
    ew, eb = _rel_t(ow.cpu(), rw), _rel_t(ob.cpu(), rb)
    print('kf %d ups %dx%d %dx%d: dw %.2e db %.2e' % (kf, Hs, Ws, cin, cout, ew, eb))
    assert ew < F32_BAR and eb < F32_BAR, (cin, cout, ew, eb)
    ow2, ob2 = _run(kf, x, du, ups=1)
    assert torch.equal(ow, ow2) and torch.equal(ob, ob2)


@pytest.mark.parametrize('kf', tfc.SIZES)
def test_wgrad_kxk_accumulate_onto_nonzero_gradients(cuda, kf):
  """chan_map (the two MAPS of wgrad_form_cases), the cut form (Cin_w = Cin - 1), both values of transposed, plain and upsampled."""
  cases = [(8, 16, 'map', 0, 0), (16, 32, 'map', 1, 0), (8, 8, 'map', 1, 1), (16, 48, 'map', 0, 1),
           (4, 8, 'cut', 0, 0), (16, 32, 'cut', 1, 0), (12, 8, 'cut', 1, 1), (8, 1, 'cut', 0, 0)]
  for cin, cout, kind, tr, ups in cases:
    B, Hs, Ws = (2, 9, 33) if not ups else (2, 5, 9)
    x, du, rng = _draw(31 * cin + cout + kf + 5 * tr, B, Hs, Ws, cin, cout, ups, cuda)
    cmap, cin_w = MAPS[cin] if kind == 'map' else (None, cin - 1)
    shape_w = (kf, kf, cout, cin_w) if tr else (kf, kf, cin_w, cout)
    g0w, g0b = torch.from_numpy(rng.randn(*shape_w).astype(np.float32)).to(cuda), torch.from_numpy(rng.randn(cout).astype(np.float32)).to(cuda)
    ow, ob = _run(kf, x, du, ups=ups, acc=(cmap, cin_w, tr), g0=(g0w, g0b))
    dw, db = tfc.wgrad_ref_ups(x.cpu(), du.cpu(), kf) if ups else tfc.wgrad_ref(x, du, kf)
    dw, db = dw.to(cuda), db.to(cuda)
    rows = cmap if cmap is not None else [ci if ci < cin_w else -1 for ci in range(cin)]
    gw = g0w.double().clone()
    for ci, j in enumerate(rows):
      if j < 0:
        continue
      if tr:  # [kf,kf,Cout,cin_w], taps flipped
        gw[:, :, :, j] += dw[:, :, ci, :].flip(0, 1)
      else:
        gw[:, :, j, :] += dw[:, :, ci, :]
    ew, eb = _rel_t(ow, gw), _rel_t(ob, g0b.double() + db)
    print('kf %d acc %dx%d %s tr %d ups %d: gw %.2e gb %.2e' % (kf, cin, cout, kind, tr, ups, ew, eb))
    assert ew < F32_BAR and eb < F32_BAR, (cin, cout, kind, tr, ups, ew, eb)
    ow2, ob2 = _run(kf, x, du, ups=ups, acc=(cmap, cin_w, tr), g0=(g0w, g0b))
    assert torch.equal(ow, ow2) and torch.equal(ob, ob2)
  # the wrappers are these entries
  x, du, _ = _draw(5, 2, 9, 33, 8, 16, 0, cuda)
  dw, db = ops.wgrad_kxk(x, du, kf)
  ow, ob = _run(kf, x, du)
  assert torch.equal(dw, ow) and torch.equal(db, ob)
  gw = torch.zeros(kf, kf, 8, 16, device=cuda)
  assert torch.equal(ops.wgrad_kxk_acc(x, du, kf, gw, torch.zeros(16, device=cuda)), ow)


def test_three_forwards_to_the_3x3_entries(cuda):
  x, du, _ = _draw(9, 2, 9, 33, 16, 32, 0, cuda)
  a = ops.wgrad_kxk(x, du, 3)
  lib = rn.lib()
  nws = lib.ra_conv3x3_wgrad_workspace_floats(16, 32, 2, 9, 33)
  ws, dw, db = torch.empty(nws, device=cuda), torch.empty(3, 3, 16, 32, device=cuda), torch.empty(32, device=cuda)
  rn.check(lib.ra_conv3x3_wgrad_f32(rn.ptr(x), 16, 2, 9, 33, 0, rn.ptr(du), 32, rn.ptr(ws), nws, rn.ptr(dw), rn.ptr(db), rn.stream_ptr()), 'wgrad')
  assert torch.equal(a[0], dw) and torch.equal(a[1], db)


def test_every_launch_form_was_reached(cuda):
  """The chooser's one variable is NT (ra_convkxk_wgrad_plan): the cases above must have run both values at every size.  (Alone,
  this test launches its own.)"""
  for kf in tfc.SIZES:
    if _FORMS.get(kf) != {1, 2}:
      for cin, cout in [(4, 8), (16, 48)]:
        _run(kf, *_draw(1, 1, 8, 32, cin, cout, 0, cuda)[:2])
    assert _FORMS[kf] == {1, 2}, (kf, _FORMS.get(kf))


def test_pack_dev_and_subsample_even(cuda):
  rng = np.random.RandomState(4)
  for kf in (1, 3, 5, 7):
    for tr in (False, True):
      w = rng.randn(kf, kf, 8, 13).astype(np.float32) if tr else rng.randn(kf, kf, 13, 8).astype(np.float32)
      cmap = list(rng.permutation(13)) + [-1] * 3
      host = ops.pack_conv_weights(w, cin_kernel=16, chan_map=cmap, transposed=tr)
      dev = ops.pack_conv_weights_dev(torch.from_numpy(w).to(cuda), kf, cin_kernel=16, chan_map=torch.tensor(cmap, dtype=torch.int32, device=cuda),
                                      transposed=tr)
      assert np.array_equal(dev.cpu().numpy(), host), (kf, tr)
  x = torch.from_numpy(rng.randn(2, 6, 10, 5).astype(np.float32)).to(cuda)
  y = torch.full((2, 3, 5, 5), float('nan'), device=cuda)
  rn.check(rn.lib().ra_subsample_even_f32(rn.ptr(x), 2, 3, 5, 5, rn.ptr(y), rn.stream_ptr()), 'ra_subsample_even_f32')
  assert torch.equal(y, x[:, ::2, ::2].contiguous())


# ---- layer level: test_train_gpu.test_conv_layer_forward_backward at the other sizes, its bars

def _rel(a, b):
  return float(np.abs(a - b).max() / max(1e-7, np.abs(b).max()))


@pytest.mark.parametrize('kf', tfc.SIZES)
def test_conv_layer_forward_backward_kxk(cuda, kf):
  import torch.nn.functional as F
  rng = np.random.RandomState(kf)
  for (cin, cout, pool, tr, stride, B, H, W) in [(4, 8, 1, False, 1, 2, 16, 24), (16, 32, 2, False, 1, 1, 8, 8), (32, 16, 1, True, 2, 2, 6, 6),
                                                  (8, 8, 1, True, 1, 2, 12, 12), (8, 1, 1, True, 2, 1, 5, 7)]:
    x = rng.randn(B, H, W, cin).astype(np.float32)
    w = (rng.randn(kf, kf, cout, cin) if tr else rng.randn(kf, kf, cin, cout)).astype(np.float32) * (0.6 / kf)
    b, gam, bet = rng.randn(cout).astype(np.float32) * 0.1, rng.uniform(0.5, 1.5, cout).astype(np.float32), \
        rng.randn(cout).astype(np.float32) * 0.1
    t = lambda a, dt, dev: torch.tensor(a, dtype=dt, device=dev, requires_grad=True)
    xr, wr, br, gr, ber = [t(a, torch.float64, 'cpu') for a in (x, w, b, gam, bet)]
    if tr:
      u = tfc.deconv_ref(xr, wr, br, stride)
    else:
      u = F.conv2d(xr.permute(0, 3, 1, 2), wr.permute(3, 2, 0, 1), padding=kf // 2).permute(0, 2, 3, 1) + br
    mean = u.mean(dim=(0, 1, 2))
    var = ((u - mean) ** 2).mean(dim=(0, 1, 2))
    v = torch.relu((u - mean) * torch.rsqrt(var + 1e-3) * gr + ber)
    yr = F.max_pool2d(v.permute(0, 3, 1, 2), pool, pool).permute(0, 2, 3, 1) if pool == 2 else v
    dy = rng.randn(*yr.shape).astype(np.float32)
    (yr * torch.tensor(dy, dtype=torch.float64)).sum().backward()
    xd, wd, bd, gd, bed = [t(a, torch.float32, cuda) for a in (x, w, b, gam, bet)]
    meta = dict(transposed=tr, stride=stride, pool=pool, relu=True, chan_map=None)
    yd, md, vd = ra_train.ConvBNActPool.apply(xd, wd, bd, gd, bed, meta)
    (yd * torch.tensor(dy, device=cuda)).sum().backward()
    tag = (kf, cin, cout, pool, tr, stride)
    assert _rel(yd.detach().cpu().numpy(), yr.detach().numpy()) < 1e-4, tag
    assert _rel(md.cpu().numpy(), mean.detach().numpy()) < 1e-4 and _rel(vd.cpu().numpy(), var.detach().numpy()) < 1e-4, tag
    for name, a, r in (('dx', xd, xr), ('dw', wd, wr), ('db', bd, br), ('dgamma', gd, gr), ('dbeta', bed, ber)):
      got, ref = a.grad.cpu().numpy(), r.grad.numpy()
      if name == 'db':  # a bias in front of BatchNorm has zero gradient: both are round-off
        assert np.abs(got - ref).max() < 1e-3 * max(1.0, np.abs(dy).sum() ** 0.5), (tag, name)
      else:
        assert _rel(got, ref) < 2e-3, (tag, name, _rel(got, ref))
    # the accumulate mode (views of a gradient bucket, a chan_map): the same sums, added
    if not tr:
      gw, gb, gg, gbt = (torch.ones_like(a) for a in (wd, bd, gd, bed))
      xd2 = torch.tensor(x, device=cuda, requires_grad=True)
      meta2 = dict(meta, grads=(gw, gb, gg, gbt))
      y2, _, _ = ra_train.ConvBNActPool.apply(xd2, wd.detach().requires_grad_(True), bd.detach().requires_grad_(True),
                                              gd.detach().requires_grad_(True), bed.detach().requires_grad_(True), meta2)
      (y2 * torch.tensor(dy, device=cuda)).sum().backward()
      assert _rel((gw - 1).cpu().numpy(), wr.grad.numpy()) < 2e-3 and _rel((gg - 1).cpu().numpy(), gr.grad.numpy()) < 2e-3, tag
      assert _rel(xd2.grad.cpu().numpy(), xr.grad.numpy()) < 2e-3, tag


def test_bf16_and_wide_layers_are_refused_by_name(cuda):
  x = torch.zeros(1, 8, 8, 8, device=cuda)
  w, b = torch.zeros(5, 5, 8, 8, device=cuda), torch.zeros(8, device=cuda)
  with pytest.raises(rn.RecAttendError, match='float32 only'):
    ra_train.ConvBNActPool.apply(x, w, b, None, None, dict(transposed=False, stride=1, pool=1, relu=True, chan_map=None, bf16=True))


# ---- the nnlib closures with train_any_filter=True: test_nnlib_train_gpu's cases and bars

def _t64(a, grad=True):
  return torch.tensor(np.asarray(a), dtype=torch.float64, requires_grad=grad)


def _oracle_train(fn):
  stats = {}
  ort._BN['train'], ort._BN['stats'] = True, stats
  try:
    return fn(), stats
  finally:
    ort._BN['train'], ort._BN['stats'] = False, None


def _set_bn(model, scope, nlayers, chans, ncopy, rng):
  vals = {}
  for ii in range(nlayers):
    for cp in range(ncopy):
      key = '%s_%d_%d' % (scope, ii, cp)
      c = chans[ii + 1]
      vals[key + '_gamma'] = rng.uniform(0.5, 1.5, c).astype(np.float32)
      vals[key + '_beta'] = (rng.randn(c) * 0.2).astype(np.float32)
      vals[key + '_ema_mean'] = (rng.randn(c) * 0.3).astype(np.float32)
      vals[key + '_ema_var'] = rng.uniform(0.5, 2.0, c).astype(np.float32)
  for k, v in vals.items():
    model[k].copy_(torch.from_numpy(v))
  return vals


@pytest.mark.parametrize('cin,ch,pool,B,H,W', [(3, [8, 8, 16], [1, 2, 2], 2, 24, 32), (4, [16, 32], [2, 1], 3, 16, 16),
                                                (13, [16, 16], [2, 2], 2, 16, 48)])
def test_cnn_train_mode_vs_oracle_kxk(cuda, cin, ch, pool, B, H, W):
  import nnlib as nn
  rng = np.random.RandomState(5)
  n = len(ch)
  fs = [5, 1, 7][:n]
  chans = [cin] + ch
  model = {}
  run = nn.cnn(fs, chans, pool, [nn.relu] * n, [True] * n, phase_train={'value': True}, wd=1e-4, scope='tcnn', model=model,
               train_any_filter=True)
  run.declare_copies(2)
  P = {}
  for ii in range(n):
    P['tcnn_w_%d' % ii] = (rng.randn(fs[ii], fs[ii], chans[ii], chans[ii + 1]) * (0.75 / fs[ii])).astype(np.float32)
    P['tcnn_b_%d' % ii] = (rng.randn(chans[ii + 1]) * 0.1).astype(np.float32)
    model['tcnn_w_%d' % ii].copy_(torch.from_numpy(P['tcnn_w_%d' % ii]))
    model['tcnn_b_%d' % ii].copy_(torch.from_numpy(P['tcnn_b_%d' % ii]))
  P.update(_set_bn(model, 'tcnn', n, chans, 2, rng))
  x = rng.randn(B, H, W, cin).astype(np.float32)
  for cp in range(2):
    keys = [k for k in P if not k.endswith(('_ema_mean', '_ema_var'))]
    Pt = {k: _t64(P[k], k in keys) for k in P}
    xr = _t64(x)
    hs_r, stats = _oracle_train(lambda: ort.cnn(xr, Pt, 'tcnn', n, pool, cp, True))
    cot = [rng.randn(*h.shape).astype(np.float32) for h in hs_r]
    sum((h * torch.tensor(c, dtype=torch.float64)).sum() for h, c in zip(hs_r, cot)).backward()
    for k in model:
      model[k].grad = None
      model[k].requires_grad_(not k.endswith(('_ema_mean', '_ema_var')))
    xd = torch.tensor(x, device=cuda, requires_grad=True)
    hs = run(xd)
    sum((h * torch.tensor(c, device=cuda)).sum() for h, c in zip(hs, cot)).backward()
    for ii in range(n):
      assert tuple(hs[ii].shape) == tuple(hs_r[ii].shape)
      assert _rel(hs[ii].detach().cpu().numpy(), hs_r[ii].detach().numpy()) < 2e-4, (cp, ii)
      key = 'tcnn_%d_%d' % (ii, cp)
      m_r, v_r = stats[key]
      m_d, v_d = run.batch_stats[key]
      assert _rel(m_d.cpu().numpy(), m_r.numpy()) < 1e-4 and _rel(v_d.cpu().numpy(), v_r.numpy()) < 1e-4, key
      assert _rel(model[key + '_ema_mean'].detach().cpu().numpy(), 0.9 * P[key + '_ema_mean'] + 0.1 * m_r.numpy()) < 1e-5
      assert _rel(model[key + '_ema_var'].detach().cpu().numpy(), 0.9 * P[key + '_ema_var'] + 0.1 * v_r.numpy()) < 1e-5
    assert _rel(xd.grad.cpu().numpy(), xr.grad.numpy()) < 2e-3, cp
    for k in keys:
      if '_%d_' % (1 - cp) in k and ('gamma' in k or 'beta' in k):
        continue
      got, ref = model[k].grad.cpu().numpy(), Pt[k].grad.numpy()
      if '_b_' in k:
        assert np.abs(got - ref).max() < 2e-3, k
      else:
        assert _rel(got, ref) < 3e-3, (cp, k, _rel(got, ref))


def test_dcnn_train_mode_vs_oracle_kxk(cuda, monkeypatch):
  """Sizes [5, 3, 1] at strides [2, 1, 2] with skip connections: a stride-2 layer of size 5 (the odd positions) and one of size 1
  (the even ones)."""
  import nnlib as nn
  monkeypatch.setattr(ort, 'deconv_same', tfc.deconv_ref)
  rng = np.random.RandomState(7)
  ch, unpool, skip_ch, fs = [16, 16, 8, 1], [2, 1, 2], [None, 8, 5], [5, 3, 1]
  n = 3
  model = {}
  run = nn.dcnn(fs, ch, unpool, [nn.relu] * n, [True] * n, skip_ch=skip_ch, phase_train=True, wd=None, scope='tdc', model=model,
                train_any_filter=True)
  run.declare_copies(1)
  P = {}
  for ii in range(n):
    P['tdc_w_%d' % ii] = (rng.randn(fs[ii], fs[ii], ch[ii + 1], run.in_chs[ii]) * (0.75 / fs[ii])).astype(np.float32)
    P['tdc_b_%d' % ii] = (rng.randn(ch[ii + 1]) * 0.1).astype(np.float32)
    model['tdc_w_%d' % ii].copy_(torch.from_numpy(P['tdc_w_%d' % ii]))
    model['tdc_b_%d' % ii].copy_(torch.from_numpy(P['tdc_b_%d' % ii]))
  P.update(_set_bn(model, 'tdc', n, ch, 1, rng))
  B, H, W = 2, 6, 10
  x = rng.randn(B, H, W, ch[0]).astype(np.float32)
  skips = [None, rng.randn(B, 2 * H, 2 * W, 8).astype(np.float32), rng.randn(B, 2 * H, 2 * W, 5).astype(np.float32)]
  keys = [k for k in P if not k.endswith(('_ema_mean', '_ema_var'))]
  Pt = {k: _t64(P[k], k in keys) for k in P}
  xr = _t64(x)
  sk_r = [None if s is None else _t64(s) for s in skips]
  hs_r, stats = _oracle_train(lambda: ort.dcnn(xr, Pt, 'tdc', n, unpool, 0, sk_r, True))
  cot = [rng.randn(*h.shape).astype(np.float32) for h in hs_r]
  sum((h * torch.tensor(c, dtype=torch.float64)).sum() for h, c in zip(hs_r, cot)).backward()
  for k in model:
    model[k].requires_grad_(not k.endswith(('_ema_mean', '_ema_var')))
  xd = torch.tensor(x, device=cuda, requires_grad=True)
  sk_d = [None if s is None else torch.tensor(s, device=cuda, requires_grad=True) for s in skips]
  hs = run(xd, skip=sk_d)
  sum((h * torch.tensor(c, device=cuda)).sum() for h, c in zip(hs, cot)).backward()
  for ii in range(n):
    assert tuple(hs[ii].shape) == tuple(hs_r[ii].shape)
    assert _rel(hs[ii].detach().cpu().numpy(), hs_r[ii].detach().numpy()) < 2e-4, ii
    key = 'tdc_%d_0' % ii
    assert _rel(run.batch_stats[key][0].cpu().numpy(), stats[key][0].numpy()) < 1e-4
    assert _rel(run.batch_stats[key][1].cpu().numpy(), stats[key][1].numpy()) < 1e-4
    assert _rel(model[key + '_ema_mean'].detach().cpu().numpy(), 0.9 * P[key + '_ema_mean'] + 0.1 * stats[key][0].numpy()) < 1e-5
    assert _rel(model[key + '_ema_var'].detach().cpu().numpy(), 0.9 * P[key + '_ema_var'] + 0.1 * stats[key][1].numpy()) < 1e-5
  assert _rel(xd.grad.cpu().numpy(), xr.grad.numpy()) < 2e-3
  for i in (1, 2):
    assert _rel(sk_d[i].grad.cpu().numpy(), sk_r[i].grad.numpy()) < 2e-3, i
  for k in keys:
    got, ref = model[k].grad.cpu().numpy(), Pt[k].grad.numpy()
    if '_b_' in k:
      assert np.abs(got - ref).max() < 2e-3, k
    else:
      assert _rel(got, ref) < 3e-3, (k, _rel(got, ref))


# ---- the whole step

@pytest.fixture(scope='module')
def full_case():
  """The inputs and the float64 oracle's answer, computed once for the tests below and left unchanged."""
  saved = ort.deconv_same
  ort.deconv_same = tfc.deconv_ref
  try:
    opt, P, x, y_gt, s_gt = tfc.step_case()
    head, gref, stats = tfc.oracle_grads(opt, P, x, y_gt, s_gt)
  finally:
    ort.deconv_same = saved
  return opt, P, x, y_gt, s_gt, head, gref, stats


def test_full_model_loss_and_every_gradient_vs_oracle(cuda, full_case):
  import full_model
  from test_train_gpu import _compare_grads
  opt, P, x, y_gt, s_gt, head, gref, stats = full_case
  m = full_model.get_model(opt).load_weights(P)
  ts = ra_train.TrainStep(m)
  assert ts.any_filter and not ts._batched_ok({})  # the per-timestep graph
  ts.bucket.zero_grad()
  loss, pieces, st = ts.forward_loss(x, y_gt, s_gt)
  loss.backward()
  for k in ('loss', 'iou_soft', 'iou_soft_box', 'conf_loss'):
    got, ref = float(pieces[k].detach()), float(head[k].detach())
    print(k, got, ref)
    assert abs(got - ref) < 2e-4 * max(1.0, abs(ref)), k
  assert (pieces['match'].cpu().numpy() == head['match'].numpy()).all()
  for key, (mean, var) in stats.items():
    assert _rel(st[key][0].cpu().numpy(), mean.numpy()) < 1e-3 and _rel(st[key][1].cpu().numpy(), var.numpy()) < 1e-3, key
  cos, worst = _compare_grads(gref, lambda k: ts.bucket.grad_of[k].cpu().numpy(), P, float(opt['weight_decay']))
  print('gradient cosine %.6f, worst per-tensor relative error %.3f' % (cos, worst))


def test_box_model_loss_and_every_gradient_vs_oracle(cuda, monkeypatch):
  import box_model
  from test_train_gpu import _compare_grads
  monkeypatch.setattr(ort, 'deconv_same', tfc.deconv_ref)
  opt, P, x, y_gt, s_gt = tfc.step_case('box', seed=7)
  noise = np.random.RandomState(9).uniform(0, 0.3, (2, 2, 64, 64)).astype(np.float32)
  head, gref, _ = tfc.oracle_grads(opt, P, x, y_gt, s_gt, noise=noise)
  m = box_model.get_model(opt).load_weights(P)
  ts = ra_train.BoxTrainStep(m)
  ts.bucket.zero_grad()
  loss, pieces, _ = ts.forward_loss(x, y_gt, s_gt, knobs={'noise': noise})
  loss.backward()
  for k in ('loss', 'box_loss', 'conf_loss', 'iou_soft_box'):
    assert abs(float(pieces[k]) - float(head[k])) < 3e-4 * max(1.0, abs(float(head[k]))), k
  assert (pieces['match_box'].cpu().numpy() == head['match_box'].numpy()).all()
  _compare_grads(gref, lambda k: ts.bucket.grad_of[k].cpu().numpy(), P, float(opt['weight_decay']))


def test_two_optimizer_steps_move_every_filter(cuda, full_case):
  """m.run(['loss', 'train_step'], feed) twice (the second step is the captured one): every conv filter moves, the 7x7 ones
  included, and the second loss is the oracle's loss at the weights the first step left."""
  import full_model
  opt, P, x, y_gt, s_gt, head, _, _ = full_case
  m = full_model.get_model(opt).load_weights(P)
  feed = {'x': x, 'y_gt': y_gt, 's_gt': s_gt, 'phase_train': True, 'aug': False}
  loss1 = float(m.run(['loss', 'train_step'], feed)[0])
  assert abs(loss1 - float(head['loss'])) < 2e-4 * max(1.0, abs(float(head['loss'])))
  P1 = {k: np.array(v) for k, v in m.state_dict_numpy().items()}
  loss2 = float(m.run(['loss', 'train_step'], feed)[0])
  P2 = m.state_dict_numpy()
  sizes = set()
  for scope, fs in (('ctrl_cnn', tfc.CTRL), ('attn_cnn', tfc.ATTN), ('attn_dcnn', tfc.DCNN)):
    for i, f in enumerate(fs):
      k = '%s_w_%d' % (scope, i)
      assert P1[k].shape[:2] == (f, f)
      for a, b in ((P[k], P1[k]), (P1[k], P2[k])):
        moved = np.abs(a - b)
        assert np.isfinite(b).all() and moved.max() <= 1.05e-3 and (moved > 0).mean() > 0.5, (k, moved.max(), (moved > 0).mean())
      sizes.add(f)
  assert sizes == {1, 3, 5, 7} and float(m['global_step']) == 2.0
  saved = ort.deconv_same
  ort.deconv_same = tfc.deconv_ref
  try:
    fwd, _ = ort.forward(opt, P1, x, phase_train=True, bn_stats={})
    ref2 = float(ort.loss_head(opt, fwd, y_gt, s_gt)['loss'])
  finally:
    ort.deconv_same = saved
  print('losses', loss1, loss2, 'oracle at the first step\'s weights', ref2)
  assert abs(loss2 - ref2) < 2e-4 * max(1.0, abs(ref2))


def test_train_cli_then_eval_cli_mixed_sizes(cuda, tmp_path, capsys):
  """full_model_train.py --train_any_filter with mixed sizes, --save_ckpt -> full_model_eval.py decodes the checkpoint (the
  scheme of test_train_gpu.test_train_cli_then_eval_cli); without the flag the same command line is refused."""
  import yaml
  import full_model_eval
  import full_model_train
  from test_train_gpu import CVPPP_FLAGS
  flags = list(CVPPP_FLAGS)
  for name, fs in (('--ctrl_cnn_filter_size', tfc.CTRL), ('--attn_cnn_filter_size', tfc.ATTN), ('--attn_dcnn_filter_size', tfc.DCNN)):
    flags[flags.index(name) + 1] = ','.join(map(str, fs))
  res = str(tmp_path / 'results')
  common = ['--results', res, '--inp_height', '64', '--inp_width', '64', '--timespan', '3', '--batch_size', '2', '--num_steps', '2',
            '--steps_per_log', '1', '--save_ckpt', '--steps_per_ckpt', '1'] + flags
  with pytest.raises(rn.RecAttendError, match='--train_any_filter'):
    full_model_train.main(common + ['--model_id', 'refused'])
  capsys.readouterr()
  full_model_train.main(common + ['--model_id', 'mix', '--train_any_filter'])
  out = capsys.readouterr().out
  losses = [float(l.split('loss')[1].split()[0]) for l in out.splitlines() if l.startswith('step ')]
  assert len(losses) == 2 and all(np.isfinite(losses))
  with open(str(tmp_path / 'results' / 'mix' / 'model_opt.yaml')) as f:
    saved = yaml.safe_load(f)
  assert saved['train_any_filter'] is True and list(saved['attn_dcnn_filter_size']) == tfc.DCNN
  w0 = dict(np.load(str(tmp_path / 'results' / 'mix' / 'weights.npz')))
  assert all(np.isfinite(v).all() for v in w0.values()) and w0['ctrl_cnn_w_4'].shape[:2] == (7, 7)
  assert float(np.abs(w0['ctrl_cnn_4_0_ema_var']).sum()) > 0
  full_model_eval.main(['--model_id', 'mix', '--results', res, '--num_synthetic', '2', '--batch_size', '2'])
  pred = np.load(str(tmp_path / 'results' / 'mix' / 'output_valid' / 'pred_rank0.npz'))
  assert pred['y_out'].shape == (2, 3, 64, 64) and np.isfinite(pred['y_out']).all()
