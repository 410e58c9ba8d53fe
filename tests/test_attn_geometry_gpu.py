"""The Gaussian-attention kernels against the float64 oracle over the window geometries the controller can emit and over every
launch form of the paste (tests/attn_geometry_cases.py; tests/test_attn_geometry.py proves on the host that the references are
conditioned eight times inside the tolerances used here and that the grid can fail).  One case is one shape; a launch holds six
records of different geometry classes.  Every case prints its worst error over tolerance per geometry class
(tools/attn_geometry_report.py collects them)."""
import numpy as np
import pytest
import torch

import attn_geometry_cases as ag
import ra_oracle as ora
import ra_ops as ops

pytestmark = pytest.mark.gpu

SENT = 7.0  # what output buffers hold before a launch: an element no workgroup wrote shows
Y_DEAD = 1.0 / (1.0 + np.exp(-ag.BETA))
B = ag.B_LAUNCH


def dev(a, cuda):
  return torch.tensor(np.ascontiguousarray(a), device=cuda)


def _batches(ref):
  n = ref['rec'].shape[0]
  return [(k, slice(k * B, (k + 1) * B)) for k in range(n // B)]


class Worst:
  """Worst error / tolerance per geometry class of a case (a record counts for its y class and its x class)."""

  def __init__(self, sid, entry):
    self.sid, self.entry, self.by_class = sid, entry, {}

  def add(self, pairs, ratio):
    for p, r in zip(pairs, np.broadcast_to(ratio, (len(pairs),))):
      for c in set(p):
        self.by_class[c] = max(self.by_class.get(c, 0.0), float(r))

  def check(self, plans=()):
    print('ATTN_GEOMETRY %s %s plans=%s %s' % (self.sid, self.entry, '|'.join(sorted(set(plans))).replace(' ', '_') or '-',
                                               ' '.join('%s=%.3f' % kv for kv in sorted(self.by_class.items()))))
    bad = {c: r for c, r in self.by_class.items() if not r < 1.0}
    assert not bad, (self.sid, self.entry, bad)


def _per_record(a):
  a = np.asarray(a, np.float64)
  return np.abs(a).reshape(a.shape[0], -1).max(axis=1)


# ---- extract ------------------------------------------------------------------------------------------------------------------
# (canvas as its own plane, use_gamma, (chan0, Cp, canvas_chan)): the whole image or its second channel group, the canvas
# standing in for a channel of the first or of the second group
EXTRACT_VARIANTS = ((0, 1, (0, 8, 3)), (1, 1, (0, 8, 3)), (1, 0, (4, 4, 5)), (0, 1, (4, 4, 5)), (1, 1, (0, 8, 5)), (0, 0, (0, 8, 5)),
                    (1, 0, (0, 8, 3)), (0, 0, (4, 4, 6)))


def _extract_ref(ref, sl, use_gamma, chans, canvas_chan):
  e = np.array(ref['extract'][sl])
  e[..., canvas_chan] = e[..., 8]
  e = e[..., chans]
  return e * ref['rec'][sl, 6].astype(np.float64).reshape(-1, 1, 1, 1) if use_gamma else e


@pytest.mark.parametrize('sid', tuple(ag.all_shapes()))
def test_extract_direct(cuda, sid):
  """ra_extract_direct_f32: every record; the canvas as a channel and as a plane, with and without gamma, the whole image and
  its second channel group (chan0 = 4), the canvas in either group; every output element written; a window wholly outside
  the image gives exactly 0."""
  H, W, Fh, Fw = ag.all_shapes()[sid]
  ref = ag.reference(sid)
  worst = Worst(sid, 'extract_direct')
  batches = _batches(ref)
  todo = [(k, sl, v) for k, sl in batches for v in (EXTRACT_VARIANTS if len(batches) == 1 else [EXTRACT_VARIANTS[(k + len(sid)) % 8]])]
  for k, sl, (plane, use_gamma, (chan0, Cp, cchan)) in todo:
    img = np.array(ref['img'][sl])
    if plane:
      img[..., cchan] = -50.0   # with a plane, that channel of the image is not read
    else:
      img[..., cchan] = ref['canvas'][sl]
    patch = torch.full((B, Fh, Fw, Cp), SENT, dtype=torch.float32, device=cuda)
    ops.extract_direct(dev(img, cuda), chan0, dev(ref['rec'][sl], cuda), Fh, Fw, Cp, use_gamma, patch,
                       canvas=dev(ref['canvas'][sl], cuda) if plane else None, canvas_chan=cchan if plane else -1)
    torch.cuda.synchronize()
    got = patch.cpu().numpy()
    want = _extract_ref(ref, sl, use_gamma, list(range(chan0, chan0 + Cp)), cchan)
    tol = ag.TOL_EXTRACT * np.maximum(1.0, _per_record(want))
    worst.add(ref['pairs'][sl], _per_record(got - want) / tol)
    out = ref['outside'][sl]
    assert (got[out] == 0.0).all(), (sid, k, 'a window outside the image')
  worst.check()


@pytest.mark.parametrize('sid', tuple(s for s, d in ag.all_shapes().items() if d[3] <= 64))
def test_extract_conv0(cuda, sid):
  """ra_extract_conv0_f32 on the same records: the patch against the oracle, layer 0 against conv2d + affine + ReLU of the
  oracle's patch."""
  H, W, Fh, Fw = ag.all_shapes()[sid]
  ref = ag.reference(sid)
  rng = np.random.RandomState(len(sid))
  worst, worst_y = Worst(sid, 'extract_conv0.patch'), Worst(sid, 'extract_conv0.y0')
  for k, sl in _batches(ref):
    plane, use_gamma, cout, chan0 = k % 2, (k // 2) % 2, (8, 12, 16)[k % 3], 4 * ((k // 4) % 2)
    cchan = chan0 + 3
    img = np.array(ref['img'][sl])
    img[..., cchan] = -50.0 if plane else ref['canvas'][sl]
    w0 = (rng.randn(3, 3, 4, cout) * 0.3).astype(np.float32)
    cp = ops.cout_padded(cout)
    sc, sh = np.ones(cp, np.float32), np.zeros(cp, np.float32)
    sc[:cout], sh[:cout] = rng.uniform(0.5, 1.5, cout), rng.randn(cout) * 0.2
    patch = torch.full((B, Fh, Fw, 4), SENT, dtype=torch.float32, device=cuda)
    y0 = torch.full((B, Fh, Fw, cout), SENT, dtype=torch.float32, device=cuda)
    ops.extract_conv0(dev(img, cuda), chan0, dev(ref['rec'][sl], cuda), Fh, Fw, use_gamma, patch, dev(w0, cuda), dev(sc, cuda),
                      dev(sh, cuda), cout, True, y0, canvas=dev(ref['canvas'][sl], cuda) if plane else None,
                      canvas_chan=cchan if plane else -1)
    torch.cuda.synchronize()
    want = _extract_ref(ref, sl, use_gamma, list(range(chan0, chan0 + 4)), cchan)
    y_ref = ora.relu(ora.conv2d(want, w0.astype(np.float64)) * sc[:cout] + sh[:cout])
    got = patch.cpu().numpy()
    worst.add(ref['pairs'][sl], _per_record(got - want) / (ag.TOL_EXTRACT * np.maximum(1.0, _per_record(want))))
    worst_y.add(ref['pairs'][sl], _per_record(y0.cpu().numpy() - y_ref) / (5e-5 * np.maximum(1.0, _per_record(y_ref))))
    assert (got[ref['outside'][sl]] == 0.0).all()
  worst.check()
  worst_y.check()


# ---- paste, box ---------------------------------------------------------------------------------------------------------------
class YBuffer:
  """y_out as the tests hand it over: plane 1 of a [B, 2, H, W]-like buffer filled with `fill`; odd: a batch stride that is no
  multiple of 4; unaligned: the plane starts 4 bytes off a 16-byte boundary."""

  def __init__(self, cuda, H, W, fill, odd=False, unaligned=False):
    self.n, self.fill = H * W, np.float32(fill)
    self.stride = ag.odd_stride(H, W) if odd else 2 * H * W
    self.off = H * W + (1 if unaligned else 0)
    self.buf = torch.full((B * self.stride + 8,), float(fill), dtype=torch.float32, device=cuda)
    self.ptr = self.buf.data_ptr() + 4 * self.off
    self.shape = (H, W)

  def planes(self):
    """The written planes [B,H,W]; asserts that nothing else in the buffer changed."""
    flat = self.buf.cpu().numpy().copy()
    out = np.stack([flat[b * self.stride + self.off:b * self.stride + self.off + self.n] for b in range(B)])
    for b in range(B):
      flat[b * self.stride + self.off:b * self.stride + self.off + self.n] = self.fill
    assert (flat == self.fill).all(), 'the launch wrote outside its y_out planes'
    return out.reshape((B,) + self.shape)


def _plan_of(sid, variant, ybuf, *tensors):
  """The plan ra_paste_plan returns for this very launch (its real alignment and stride), as the case table names plans."""
  H, W, Fh, Fw = ag.all_shapes()[sid]
  v = dict(ag.PASTE_VARIANTS[variant])
  v.pop('odd_stride', None)
  v.pop('aligned16', None)
  a16 = all(p % 16 == 0 for p in [ybuf.ptr] + [t.data_ptr() for t in tensors if t is not None])
  p = ops.paste_plan(v.pop('mode'), B, H, W, Fh, Fw, y_stride_b=ybuf.stride, aligned16=a16, **v)
  return '%s r%d %s' % (p['kernel'], p['rows'], 'short' if H % p['rows'] else 'full')


FLAG_MODES = (0, ops.PASTE_Y_PREFILLED, ops.PASTE_Y_PREFILLED | ops.PASTE_CANVAS_FLOORED)


def _paste_launch(cuda, sid, ref, sl, variant, overwrite, flags, score=None):
  """One paste of records sl in the given variant.  Returns (y [B,H,W], canvas after or None, canvas before, plan)."""
  H, W, Fh, Fw = ag.all_shapes()[sid]
  v = ag.PASTE_VARIANTS[variant]
  y_dead32 = np.float32(1.0) / (np.float32(1.0) + np.exp(np.float32(-ag.BETA)))
  c0 = np.array(ref['canvas'][sl])
  if flags == ops.PASTE_Y_PREFILLED:
    c0[:] = 0.0                          # the first paste of a forward
  elif flags:
    c0 = np.maximum(c0, y_dead32)        # a canvas the earlier pastes floored
  ybuf = YBuffer(cuda, H, W, y_dead32 if flags else SENT, odd=v.get('odd_stride', False), unaligned=not v.get('aligned16', True))
  Cp, pc = v['Cp'], v['pc']
  P = np.random.RandomState(7).randn(B, Fh, Fw, Cp).astype(np.float32) * 100.0   # the other patch channels are not read
  P[..., pc] = ref['P'][sl]
  dP, drec = dev(P, cuda), dev(ref['rec'][sl], cuda)
  dcv = dev(c0, cuda) if v['has_canvas'] else None
  img0 = dimg = None
  if v['has_img']:
    img0 = np.array(ref['img'][sl])
    img0[..., 3] = c0
    dimg = dev(img0, cuda)
  plan = _plan_of(sid, variant, ybuf, dP, dcv)
  assert plan == ag.PASTE_CASES[sid][variant], (sid, variant, plan)
  if score is None:
    ops.paste_direct(dP, pc, drec, ag.BETA, overwrite, ybuf.ptr, ybuf.stride, H, W, canvas=dcv, img=dimg,
                     canvas_chan=3 if v['has_img'] else -1, flags=flags)
  else:
    h, core, w, bias, s_buf, s_stride = score
    ops.paste_score_direct(dP, pc, drec, ag.BETA, overwrite, ybuf.ptr, ybuf.stride, H, W, dcv, flags, h, core, w, bias, s_buf, s_stride)
  torch.cuda.synchronize()
  y = ybuf.planes()
  cv = None
  if v['has_canvas']:
    cv = dcv.cpu().numpy()
  elif v['has_img']:
    gi = dimg.cpu().numpy()
    cv = gi[..., 3]
    keep = [0, 1, 2, 4, 5, 6, 7]
    assert (gi[..., keep] == img0[..., keep]).all(), 'the paste touched an image channel other than the canvas'
  return y, cv, (c0 if (v['has_canvas'] or v['has_img']) else np.zeros_like(c0)), plan


def _check_paste(worst, ref, sl, y, cv, c0, overwrite, has_canvas):
  yy = ref['paste'][sl]
  want = yy * (1.0 - c0.astype(np.float64)) if (overwrite and has_canvas) else yy
  ratio = _per_record(y - want) / ag.TOL_PASTE
  if cv is not None:
    ratio = np.maximum(ratio, _per_record(cv - np.maximum(want, c0)) / ag.TOL_PASTE)
  worst.add(ref['pairs'][sl], ratio)
  out = ref['outside'][sl]
  dead = Y_DEAD * (1.0 - c0.astype(np.float64)) if (overwrite and has_canvas) else np.full(c0.shape, Y_DEAD)
  assert np.abs(y[out] - dead[out]).max(initial=0.0) <= 1e-7, 'a window outside the image: y = sigmoid(beta) on the whole plane'


# the form-only rows run the decode loop's launch only
PASTE_PARAMS = [(sid, form) for sid in ag.PASTE_CASES for form in ('plane', 'chan', 'packed') if form == 'plane' or sid not in ag.FORM_ROWS]


@pytest.mark.parametrize('sid,form', PASTE_PARAMS)
def test_paste_direct(cuda, sid, form):
  """ra_paste_direct_f32 in one form of its arguments (canvas plane / canvas as an image channel / canvas plane with patch
  channel 2 of 4) on every record: disable_overwrite 0 and 1; flags 0, Y_PREFILLED alone from a zero canvas, Y_PREFILLED |
  CANVAS_FLOORED on a floored canvas; y_out and canvas against the oracle, nothing else written, and the kernel the case table
  names.  The plane form adds the launches that leave the window kernel by one condition each: a y_out view of odd batch
  stride, one off 16-byte alignment, and no canvas at all."""
  ref = ag.reference(sid)
  worst, plans = Worst(sid, 'paste_direct.' + form), []
  batches = _batches(ref)
  combos = [(o, f) for f in FLAG_MODES for o in (0, 1)]
  fi = ('plane', 'chan', 'packed').index(form)
  todo = [(k, sl, c) for k, sl in batches for c in (combos if len(batches) == 1 else [combos[(k + fi) % 6]])]
  for k, sl, (overwrite, flags) in todo:
    y, cv, c0, plan = _paste_launch(cuda, sid, ref, sl, form, overwrite, flags)
    _check_paste(worst, ref, sl, y, cv, c0, overwrite, True)
    plans.append(plan)
  if form == 'plane' and sid not in ag.FORM_ROWS:
    for j, variant in enumerate(('stride', 'unaligned', 'nocanvas')):
      for k, sl in batches[2 * j:2 * j + 2]:
        overwrite, flags = combos[(k + 1) % 6]
        y, cv, c0, plan = _paste_launch(cuda, sid, ref, sl, variant, overwrite, flags)
        _check_paste(worst, ref, sl, y, cv, c0, overwrite, variant != 'nocanvas')
        plans.append(plan)
  worst.check(plans)


@pytest.mark.parametrize('sid', tuple(ag.PASTE_CASES))
def test_attn_box_direct(cuda, sid):
  """ra_attn_box_direct_f32 on every record, in the form the shape gives and, through a view of odd batch stride, in the
  general one."""
  H, W, Fh, Fw = ag.all_shapes()[sid]
  ref = ag.reference(sid)
  worst, plans = Worst(sid, 'attn_box_direct'), []
  for variant in ('box',) if sid in ag.FORM_ROWS else ('box', 'box_stride'):
    for k, sl in _batches(ref):
      ybuf = YBuffer(cuda, H, W, SENT, odd=variant == 'box_stride')
      plan = _plan_of(sid, variant, ybuf)
      assert plan == ag.PASTE_CASES[sid][variant], (sid, variant, plan)
      ops.attn_box_direct(dev(ref['rec'][sl], cuda), H, W, Fh, Fw, ag.BETA, ybuf.ptr, ybuf.stride)
      torch.cuda.synchronize()
      got = ybuf.planes()
      worst.add(ref['pairs'][sl], _per_record(got - ref['box'][sl]) / ag.TOL_BOX)
      assert np.abs(got[ref['outside'][sl]] - Y_DEAD).max(initial=0.0) <= 1e-7
      plans.append(plan)
  worst.check(plans)


@pytest.mark.parametrize('sid,variant', [('s40x72', 'plane'), ('s22x40', 'plane'), ('s37x50', 'plane'), ('s40x72', 'packed')])
def test_paste_score_direct(cuda, sid, variant):
  """ra_paste_score_direct_f32: y_out and canvas bit-for-bit those of ra_paste_direct_f32 on the same arguments, the score of the
  rider workgroup against sigmoid([h | core] . w + b) in float64; with and without a core part, s_out dense and strided; in the
  window form (all rows, a short last block) and the general form (W % 4 != 0; a packed patch channel)."""
  ref = ag.reference(sid)
  rng = np.random.RandomState(11)
  worst, plans = Worst(sid, 'paste_score_direct.' + variant), []
  combos = [(o, f) for f in FLAG_MODES for o in (0, 1)]
  for k, sl in _batches(ref):
    overwrite, flags = combos[k % 6]
    K0, K1, s_stride = (300, 70, 37)[k % 3], (0, 33)[k % 2], (1, 3)[(k // 2) % 2]
    h, w, bias = rng.randn(B, K0).astype(np.float32), (rng.randn(K0 + K1) / 8).astype(np.float32), rng.randn(1).astype(np.float32)
    core = rng.randn(B, K1).astype(np.float32) if K1 else None
    s_buf = torch.full((B * s_stride,), SENT, dtype=torch.float32, device=cuda)
    score = (dev(h, cuda), None if core is None else dev(core, cuda), dev(w, cuda), dev(bias, cuda), s_buf, s_stride)
    y1, cv1, c0, plan = _paste_launch(cuda, sid, ref, sl, variant, overwrite, flags, score=score)
    y0, cv0, _, plan0 = _paste_launch(cuda, sid, ref, sl, variant, overwrite, flags)
    assert plan == plan0 and (y1 == y0).all() and (cv1 == cv0).all()
    _check_paste(worst, ref, sl, y1, cv1, c0, overwrite, True)
    x = h.astype(np.float64) if core is None else np.concatenate([h, core], 1).astype(np.float64)
    s_ref = ora.sigmoid(x @ w.astype(np.float64) + bias[0])
    s = s_buf.cpu().numpy().reshape(B, s_stride)
    assert np.abs(s[:, 0] - s_ref).max() < 2e-5 and (s[:, 1:] == SENT).all()
    plans.append(plan)
  worst.check(plans)


# ---- the dense bank -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('sid', tuple(ag.SHAPES))
def test_gaussian_filter_bank(cuda, sid):
  """ra_gaussian_filter_f32 on every record, per record and axis at the existing bound (the error over the bank's largest
  weight, or over 1e-6 where the bank is smaller); a bank wholly below 1e-30 is held to that absolutely."""
  H, W, Fh, Fw = ag.all_shapes()[sid]
  ref = ag.reference(sid)
  rec = ref['rec']
  worst = Worst(sid, 'gaussian_filter')
  for axis, (L, F, bank) in enumerate(((H, Fh, ref['fy']), (W, Fw, ref['fx']))):
    col = lambda c: dev(rec[:, c + axis], cuda)
    got = ops.gaussian_filter(col(0), col(2), col(4), L, F).cpu().numpy()
    err, top = _per_record(got - bank), _per_record(bank)
    tiny = top < 1e-30
    assert (err[tiny] < 1e-30).all()
    ratio = np.where(tiny, 0.0, err / np.maximum(1e-6, top) / 1e-4)
    worst.add([(p[axis],) for p in ref['pairs']], ratio)   # a bank belongs to its own axis' class
  worst.check()


# ---- adjoints -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('sid', tuple(ag.ADJOINT_SHAPES))
def test_resample_adjoints(cuda, sid):
  """ra_resample_bwd_f32 in its READ / BOX / WRITE modes, as the backward of ra_train.AttnExtract / AttnPaste, against float64
  torch autograd of the dense formulation, per record and parameter; the forward values too.  A window wholly outside the
  image has finite gradients within tolerance of the (vanishing) reference."""
  import ra_train
  case = ag.adjoint_case(sid)
  H, W, Fh, Fw = case['dims']
  worst, worst_f = Worst(sid, 'resample_bwd'), Worst(sid, 'resample_fwd')
  n = case['rec'].shape[0]
  for lo in range(0, n, B):
    sl = slice(lo, lo + B)
    fwd, g_ref = ag.adjoint_reference(case, lo, lo + B, torch.float64)
    rec = case['rec'][sl]
    leaf = lambda a: dev(a, cuda).requires_grad_(True)
    ctr, size, lgv = leaf(rec[:, 0:2]), leaf(rec[:, 2:4]), leaf(rec[:, 4:6])
    g_e, g_b, g_y, P = leaf(rec[:, 6]), leaf(rec[:, 7]), leaf(rec[:, 8]), leaf(case['P'][sl])
    e = ra_train.AttnExtract.apply(dev(case['x'][sl], cuda), ctr, size, lgv, g_e, Fh, Fw)
    bx = ra_train.AttnPaste.apply(None, ctr, size, lgv, g_b, H, W, Fh, Fw)
    y = ra_train.AttnPaste.apply(P[..., None], ctr, size, lgv, g_y, H, W, Fh, Fw)
    ((e * dev(case['wE'][sl], cuda)).sum() + (bx * dev(case['wB'][sl], cuda)).sum() + (y * dev(case['wY'][sl], cuda)).sum()).backward()
    torch.cuda.synchronize()
    got = {k: t.grad.cpu().numpy() for k, t in zip(ag.ADJOINT_PARAMS, (ctr, size, lgv, g_e, g_b, g_y, P))}
    excess, at = ag.adjoint_excess(got, g_ref)
    worst.add(case['pairs'][sl], excess)
    assert (excess < 1.0).all(), [(case['pairs'][lo + i], at[i], excess[i]) for i in np.flatnonzero(~(excess < 1.0))]
    for a, r, tol in zip((e, bx, y), fwd, (ag.TOL_EXTRACT, ag.TOL_BOX, ag.TOL_PASTE)):
      scale = np.maximum(1.0, _per_record(r)) if tol == ag.TOL_EXTRACT else 1.0
      worst_f.add(case['pairs'][sl], _per_record(a.detach().cpu().numpy() - r) / (tol * scale))
  worst.check()
  worst_f.check()
