"""One conv + BatchNorm + ReLU + pool layer of nnlib.cnn (nnlib.py:229-253) / nnlib.dcnn (nnlib.py:362-400) in training mode, as
autograd nodes over the HIP kernels (ra_ops), for ra_train, ra_fg_train and the train-mode nnlib closures: ConvBNActPool (one call,
one packed input), ConvStackFn (a layer's T calls stacked: backward only), WideConvBNActPool (beyond 128 channels, two sources),
BatchNormTrain.  Forward: operands -> conv with the batch moments -> normalise + ReLU + pool; backward: BatchNorm adjoint -> filter
gradient (deferred, added to a bucket, or fresh) -> data gradient, which is conv_dgrad for every node.  Also here: scratch, device
constants, channel padding, concat_skip, the pack caches.  Tuning aids: RA_EPI_MOMENTS=0 (two-pass moments), RA_SPLIT_DGRAD=0.
"""
import ctypes as _C
import os

import torch

import ra_dist
import ra_native as rn
import ra_ops as ops
from nnlib import WIDE_COUT
from ra_native import check, ptr
from ra_ops import _POISON, _f  # noqa: F401  (scratch: RA_POISON fills it)

# the collectives of a synchronised BatchNorm; ra_train stands its own (replaceable) names in
COLLECTIVES = {'sync_moments': ra_dist.sync_moments, 'allreduce_sums': ra_dist.allreduce_sums}


class _LatestVersionPack(dict):
  """The pack cache of callers OUTSIDE a TrainStep (the train-mode nnlib closures, tests, one-off layer calls).  Keys carry the
  source tensor's data pointer AND version — (ptr, version, geometry...), ('shift', ptr, version, cp), ('split', ptr, version,
  transposed) — so an in-place optimizer step makes every entry of that weight stale; a plain dict kept them all and an
  ordinary training loop over the closures grew by one set of packed filters per layer, direction and step (~1 MB
  per step at the CVPPP arch).  Here a new version of the same (tensor, geometry) REPLACES the old entry, and the whole cache
  is capped (oldest first) for callers that keep creating tensors."""
  CAP = 2048

  def __init__(self):
    super().__init__()
    self._latest = {}

  @staticmethod
  def _identity(key):
    return (key[0], key[1]) + tuple(key[3:]) if isinstance(key[0], str) else (key[0],) + tuple(key[2:])

  def __setitem__(self, key, value):
    ident = self._identity(key)
    old = self._latest.get(ident)
    if old is not None and old != key:
      super().pop(old, None)
    self._latest[ident] = key
    super().__setitem__(key, value)
    while len(self) > self.CAP:
      k0 = next(iter(self))
      super().pop(k0)
      self._latest.pop(self._identity(k0), None)

  def clear(self):
    super().clear()
    self._latest.clear()


_PACK = _LatestVersionPack()
# A TrainStep owns its own cache
# (TrainStep._pack, handed to the layer functions through meta['cache']): per step, (weight storage, geometry) -> packed
# filter — the filters are shared by the T timesteps.  forward_loss() clears the trainer's dict (the optimizer writes the
# weights through raw pointers); an entry keeps its source tensor alive and carries the tensor's version, so a caller
# cannot be handed the pack of a freed tensor whose address was reused, nor one that predates an in-place update.


class _PackCache(dict):
  """A TrainStep's per-step cache of packed filters (cleared by every forward_loss), plus the step's PRE-PACKED filters:
  the device packer only moves values, so packing an array of flat-bucket POSITIONS once per (layer, geometry) gives an
  index map, and every later step packs all of its filters and pads all of its biases with ONE gather launch over the
  parameter bucket (ra_gather_f32) instead of one pack launch (+ a fill and a copy for a padded bias) per layer and
  direction.  A geometry seen for the first time takes the per-layer launch and joins the map for the next step."""

  def __init__(self, trainer):
    super().__init__()
    self.tr = trainer
    self.entries, self.pending = {}, []   # key -> (start, n) in self.wp; [(key, index map)] waiting for the next refresh
    self.imap = self.wp = None
    self.filled = -1                        # the pack epoch self.wp holds

  def _where(self, t):
    """Offset (in floats) of a contiguous float32 parameter inside the bucket, or None."""
    par = self.tr.bucket.param
    off = t.data_ptr() - par.data_ptr()
    if t.dtype != torch.float32 or not t.is_contiguous() or off < 0 or off % 4 or off // 4 + t.numel() > par.numel():
      return None
    return off // 4

  def _positions(self, t, off):
    assert self.tr.bucket.param.numel() < (1 << 24)  # positions (+1; 0 = "no source") are exact in float32
    return (torch.arange(t.numel(), device=t.device, dtype=torch.float32) + float(off + 1)).reshape(t.shape)

  def lookup(self, key, t, make_map):
    """key: the packing's geometry; t: the parameter; make_map(positions) -> packed positions.  The packed values of
    this step, or None (first sight of the geometry, or a tensor outside the bucket: the caller packs as before)."""
    off = self._where(t)
    if off is None or not getattr(self.tr, 'prepack', True):
      return None
    key = (off, t.numel()) + key
    hit = self.entries.get(key)
    if hit is not None:
      return self.wp[hit[0]:hit[0] + hit[1]] if self.filled == self.tr._pack_epoch else None
    if all(k != key for k, _ in self.pending) and not torch.cuda.is_current_stream_capturing():
      with torch.no_grad():
        self.pending.append((key, (make_map(self._positions(t, off)).reshape(-1) - 1.0).to(torch.int32)))
    return None

  def merge(self):
    """Take in the geometries met since the last merge.  Never inside a stream capture: the index map is built by eager
    launches from tensors that are freed here (a captured copy of those launches would re-read freed memory at every
    replay); TrainStep._graphed merges before it captures."""
    if self.pending and not torch.cuda.is_current_stream_capturing():
      self.tr._drop_captured_steps()  # the buffers below move
      n0 = 0 if self.imap is None else self.imap.numel()
      maps = ([self.imap] if n0 else [])
      for key, m in self.pending:
        pad = (-m.numel()) % 4       # 16-byte aligned views
        self.entries[key] = (n0, m.numel())
        maps.append(torch.nn.functional.pad(m, (0, pad), value=-1))
        n0 += m.numel() + pad
      self.imap = torch.cat(maps)
      self.wp = torch.empty(n0, dtype=torch.float32, device=self.imap.device)
      self.pending = []

  def refresh(self):
    """Once per optimisation step, after the epoch moved: this step's packed filters and padded biases, one gather."""
    self.merge()
    if self.imap is not None and getattr(self.tr, 'prepack', True):
      check(rn.lib().ra_gather_f32(ptr(self.tr.bucket.param), ptr(self.imap), self.imap.numel(), ptr(self.wp), rn.stream_ptr()),
            'ra_gather_f32')
      self.filled = self.tr._pack_epoch


def _pack_dev(w, cin_w, cout, cin, cmap_t, transposed, cache=None, ksize=3):
  cache = _PACK if cache is None else cache
  key = (w.data_ptr(), w._version, int(cin_w), int(cout), int(cin), 0 if cmap_t is None else cmap_t.data_ptr(), bool(transposed))
  if ksize != 3:
    key += (int(ksize),)
  hit = cache.get(key)
  if hit is not None:
    return hit[1]
  if isinstance(cache, _PackCache):
    pre = cache.lookup(('w',) + key[2:], w, lambda pos: _pack_dev_now(pos, cin_w, cout, cin, cmap_t, transposed, ksize))
    if pre is not None:
      cache[key] = (w, pre)
      return pre
  out = _pack_dev_now(w, cin_w, cout, cin, cmap_t, transposed, ksize)
  cache[key] = (w, out)
  return out


def _pack_dev_now(w, cin_w, cout, cin, cmap_t, transposed, ksize=3):
  if ksize != 3:  # a filter of size 1, 5 or 7 (ra_convkxk_f32's packing)
    return ops.pack_conv_weights_dev(w, ksize, cin_kernel=cin, chan_map=cmap_t, transposed=transposed)
  n = rn.lib().ra_conv_packed_floats(cin, cout)
  if n == 0:
    raise rn.RecAttendError('unsupported conv shape Cin=%d Cout=%d' % (cin, cout))
  out = _f(n, device=w.device)
  check(rn.lib().ra_conv_pack_weights_dev(ptr(w), int(cin_w), int(cout), int(cin), ptr(cmap_t),
                                          rn.RA_CONV_TRANSPOSED if transposed else 0, ptr(out), rn.stream_ptr()),
        'ra_conv_pack_weights_dev')
  return out


def _cached(cache, key, w, make):
  """cache[key] = (w, make()) unless it is there: the entry keeps its source tensor alive."""
  hit = cache.get(key)
  if hit is None:
    hit = cache[key] = (w, make())
  return hit[1]


_CONST = {}


def _const(kind, key, device, make):
  """Small constant device tensors (unit scales, zero shifts, channel maps) are built once: a training
  step runs ~1300 layer calls and each host->device upload costs more than the kernel it feeds."""
  k = (kind, key, str(device))
  t = _CONST.get(k)
  if t is None:
    t = _CONST[k] = make()
  return t


def _ones_zeros(n, dev, zeros=True):
  """Unit scale and (zeros) zero shift of n floats."""
  one = _const('ones', n, dev, lambda: torch.ones(n, dtype=torch.float32, device=dev))
  return (one, _const('zeros', n, dev, lambda: torch.zeros(n, dtype=torch.float32, device=dev))) if zeros else one


def _cmap_dev(cmap, dev):
  """A channel map (list of filter rows, -1 = padding; or None) as an int32 device tensor."""
  if cmap is None:
    return None
  return _const('cmap', tuple(cmap), dev, lambda: torch.tensor(cmap, dtype=torch.int32, device=dev))


def _pad_map(n_real, n_kernel, device):
  """chan_map for a kernel input of n_kernel channels whose first n_real are real."""
  if n_real == n_kernel:
    return None
  return _const('padmap', (n_real, n_kernel), device, lambda: torch.tensor(
      list(range(n_real)) + [-1] * (n_kernel - n_real), dtype=torch.int32, device=device))


def pad4(c):
  return -(-c // 4) * 4


def _pad_channels(t, mult=4):
  c = t.shape[-1]
  cp = -(-c // mult) * mult
  if cp == c:
    return t.contiguous()
  out = torch.zeros(t.shape[:-1] + (cp,), dtype=t.dtype, device=t.device)
  out[..., :c] = t
  return out


def concat_skip(prev, skip, skip_map=None, keep_identity=False):
  """concat(prev, skip) (nnlib.py:365) as ONE packed kernel input: each side padded to a multiple of 4 channels -> (packed tensor,
  chan_map list: packed channel -> filter row, -1 = padding).  skip_map: the real channels of a skip that is itself packed.  An
  identity map says what the kernels' default says and comes back as None (it reaches the pack-cache key) unless keep_identity."""
  n_prev = prev.shape[3]
  xp, skp = _pad_channels(prev), _pad_channels(skip if skip.dtype == prev.dtype else skip.to(prev.dtype))
  skip_map = list(range(skip.shape[3])) if skip_map is None else skip_map
  cmap = list(range(n_prev)) + [-1] * (xp.shape[3] - n_prev) + [n_prev + m if m >= 0 else -1 for m in skip_map] + \
      [-1] * (skp.shape[3] - len(skip_map))
  return torch.cat([xp, skp], dim=3), (None if not keep_identity and cmap == list(range(len(cmap))) else cmap)


def _source_maps(c0, C0, c1, C1, dev):
  """Kernel channel -> filter row for a layer whose kernel input is [x0 (C0 channels, c0 real) | x1 (C1, c1 real)] and whose
  filter has c0 + c1 input rows: (the whole input's map, x0's, x1's) as int32 device tensors; None where the kernels' default
  (channel c is row c) says the same."""
  m0 = list(range(c0)) + [-1] * (C0 - c0)
  m1 = [c0 + m for m in range(c1)] + [-1] * (C1 - c1)
  whole = None if (C0 == c0 and C1 == c1) else _cmap_dev(m0 + m1, dev)
  return whole, (None if (C0 == c0 and not C1) else _cmap_dev(m0, dev)), (_cmap_dev(m1, dev) if C1 else None)


EPILOGUE_MOMENTS = {'on': os.environ.get('RA_EPI_MOMENTS', '1') != '0'}  # tuning aid: 0 = the two-pass moments kernels
SPLIT_DGRAD = {'on': os.environ.get('RA_SPLIT_DGRAD', '1') != '0'}  # tuning aid: 0 = every float32 data gradient on K1


def _padded_shift(b, cout, cp, cache):
  """The layer's bias as the conv's shift of cp floats: padded once per step (it is shared by all timesteps), not once per use."""
  if cp == cout:
    return b.detach()
  key = ('shift', b.data_ptr(), b._version, cp)
  hit = cache.get(key)
  if hit is None:
    pre = cache.lookup(('b', cp), b.detach(), lambda pos: torch.nn.functional.pad(pos, (0, cp - cout))) \
        if isinstance(cache, _PackCache) else None
    hit = cache[key] = (b, pre if pre is not None else torch.nn.functional.pad(b.detach(), (0, cp - cout)))
  return hit[1]


def _conv_moments(x, wp, scale, shift, cout, u, stride, ksize=3, bf16=False, stats=None, stored=False):
  """u = conv(x) + shift into the given tensor and, with stats = (mean, var), its batch moments into them: on the conv's epilogue
  where it has one (3x3, cout % 4 == 0), else by the two-pass kernel over u.  stored: the bf16 mode's stacked step, bf16 x and / or u."""
  ups = stride == 2
  sflags = ((1 if x.dtype == torch.bfloat16 else 0) | (2 if u.dtype == torch.bfloat16 else 0)) if stored else None
  if stats is not None and cout % 4 == 0 and EPILOGUE_MOMENTS['on'] and ksize == 3:
    _, part, nparts = ops.conv3x3_train(x, wp, scale, shift, cout, upsample=ups, bf16=bf16, out=u, store_flags=sflags)
    ops.bn_moments_from_partials(part, nparts, cout, out=stats)
    return u
  if stored:
    ops.conv3x3_train(x, wp, scale, shift, cout, upsample=ups, out=u, store_flags=sflags, moments=False)
  elif ksize == 3:
    ops.conv3x3(x, wp, scale, shift, cout, relu=False, pool=1, upsample=ups, bf16=bf16, out=u)
  else:  # ra_convkxk_f32: its epilogue carries no moments
    ops.conv2d_fused(x, wp, scale, shift, cout, ksize, relu=False, pool=1, upsample=ups, out=u)
  if stats is not None:
    ops.bn_moments(u, out=stats)
  return u


def _bn_backward(u, dy, mean, var, gamma, beta, relu, pool, acc, n_total=0.0):
  """BatchNorm / ReLU / pool adjoint of one call -> (du, dgamma, dbeta); acc = (bucket gamma, bucket beta) the kernel adds them to.
  n_total: elements per channel of the WHOLE batch under synchronised statistics (the sums cross the ranks before the du pass)."""
  B, H, W, cout = u.shape
  if not (n_total > 0.0 and n_total != float(B * H * W)):
    return ops.bn_act_pool_bwd(u, dy, mean, var, gamma, beta, relu=relu, pool=pool, acc=acc)
  both = _f(2 * cout, device=u.device)
  ops.bn_act_pool_bwd_reduce(u, dy, mean, var, gamma, beta, relu=relu, pool=pool, acc=acc or (None, None), out=(both[:cout], both[cout:]))
  mine = both.clone()
  COLLECTIVES['allreduce_sums'](both)
  du = ops.bn_act_pool_bwd_dx(u, dy, mean, var, gamma, beta, both[:cout], both[cout:], n_total, relu=relu, pool=pool)
  return du, mine[:cout], mine[cout:]


def _wgrad_fresh(x, du, ksize, stride, bf16, cmap, cin_w, transposed):
  """The filter gradient of the conv that ran, as new tensors in the reference layout of its filter -> (dw, db)."""
  if ksize != 3:
    dWf, db = ops.wgrad_kxk(x, du, ksize, upsample=(stride == 2))
  else:
    dWf, db = ops.wgrad3x3(x, du, upsample=(stride == 2), bf16=bf16)
  if cmap is not None:  # packed kernel channels -> the filter's own input channels
    real = torch.zeros((ksize, ksize, cin_w, du.shape[3]), dtype=torch.float32, device=x.device)
    for c, j in enumerate(cmap):
      if j >= 0:
        real[:, :, j, :] += dWf[:, :, c, :]
    dWf = real
  elif x.shape[3] != cin_w:
    dWf = dWf[:, :, :cin_w, :]
  return (dWf.flip(0, 1).permute(0, 1, 3, 2).contiguous() if transposed else dWf.contiguous()), db


class _DeferredWgrads(dict):
  """(scope, layer) -> the (x, du) pairs of the layer's calls in the running backward pass.  A filter shared by the
  step's T timesteps (every nnlib.cnn / dcnn layer of full_model, full_model.py:455-535) sums T filter gradients; as
  the end-of-backward callback this object forms each layer's sum in ONE pass over the images of all its calls
  (ra_conv3x3_wgrad_multi_acc_f32 through two pointer tables): 4 launches per layer and step instead of 2 T, and the
  patch-sized layers' fixed costs (launch, cross-wave reduction, partial sums) are paid once, not T times."""
  armed = False

  def reset(self):
    """A new forward pass: nothing of an interrupted backward pass may be added to."""
    self.armed = False
    for slot in self.values():
      slot['calls'] = []

  def add(self, key, x, du, shape, cmap_t, gw, gb):
    """One call of layer `key`: nothing is launched here."""
    if not self.armed:
      self.armed = True
      torch.autograd.Variable._execution_engine.queue_callback(self)
    slot = self.get(key)
    if slot is None:
      slot = self[key] = dict(calls=[], tab=torch.zeros(128, dtype=torch.int64, device=x.device), ws=None)
    assert slot.setdefault('shape', shape) == shape, 'a deferred filter gradient needs one shape per layer'
    slot['calls'].append((x, du))
    slot.update(cmap_t=cmap_t, gw=gw, gb=gb)

  def __call__(self):
    self.armed = False
    for slot in self.values():
      calls, slot['calls'] = slot['calls'], []
      Cx, cout, B, Hs, Ws, H, W, ups, _, cin_w, tr, bf = slot['shape']
      for k in range(0, len(calls), 64):
        part = calls[k:k + 64]
        n = len(part)
        nws = ops.wgrad3x3_workspace_floats(Cx, cout, n * B, H, W)
        if slot['ws'] is None or slot['ws'].numel() < nws:
          slot['ws'] = _f(nws, device=slot['tab'].device)
        tab = slot['tab']
        for off, col in ((0, 0), (64, 1)):
          host = (_C.c_void_p * n)(*[c[col].data_ptr() for c in part])
          check(rn.lib().ra_ptr_table(host, n, tab.data_ptr() + 8 * off, rn.stream_ptr()), 'ra_ptr_table')
        ops.wgrad3x3_multi_acc(tab, n, (B, Hs, Ws, Cx), cout, slot['ws'], slot['gw'], slot['gb'], chan_map=slot['cmap_t'], cin_w=cin_w,
                               transposed=tr, upsample=ups, bf16=bf)


def conv_dgrad(du, w, transposed, stride, x_shape, ksize=3, chan_map=None, rows=None, cache=None, bf16=False,
               out_dtype=torch.float32, allow_split=False):
  """The data gradient of a layer's conv: the conv kernel on the flipped, in / out-swapped packing of the filter, then (stride
  2) every second position of the full-resolution result, then back to the kernel input's channels.  du [B,H,W,>= Cout]
  (channels beyond the filter's are padding), float32 or bf16; w the layer's filter in the reference layout; x_shape =
  (B,Hs,Ws,Cx) of the kernel input the result is for.  chan_map (list: kernel channel -> filter row, -1 = padding) or rows =
  (first, n), the filter rows of one source of a two-source layer; neither: the first Cin of the Cx channels are the rows.
  Routes: K1s split (allow_split, 32 -> 32 float32, stride 1, no map or padding), K1-wide (more than 128 rows), bf16 storage
  (du or out_dtype bf16: ra_conv3x3_bf16_f32), k x k (ksize 1, 5, 7), else K1 on float32 or (bf16) bf16 operands."""
  dev = du.device
  B, Hs, Ws, Cx = x_shape
  H, W = du.shape[1], du.shape[2]
  cache = _PACK if cache is None else cache
  cout, cin_w = (w.shape[2], w.shape[3]) if transposed else (w.shape[3], w.shape[2])
  first, n = (0, cin_w) if rows is None else rows
  stored = du.dtype == torch.bfloat16 or out_dtype == torch.bfloat16
  # ---- the conv at full resolution -> dxr [B,H,W,n]
  if (allow_split and SPLIT_DGRAD['on'] and not bf16 and not stored and ksize == 3 and rows is None and stride == 1 and chan_map is None and
      Cx == cin_w and cout == 32 and du.shape[3] == cout and  # (16 channels: conv16_kernel is as fast; 64: K1s's 8-row form is the decode loop's, not measured here)
      ops.conv_split_supported(cout, cin_w, 1, H, W) and du.numel() * 4 < (1 << 31)):
    # round 5: the float32 data gradient of a 16- / 32-channel layer on the bf16 matrix pipe at float32 accuracy (K1s,
    # csrc/ra_conv_split.hip: every operand the exact sum of three bf16 pieces, six piece products) — 32 -> 32 at 128 x 128 x
    # 128 images: 2 x 292 -> 193 us in the cfg4 step.  The filter's pieces are packed on the device once per step (cache: per pack epoch).
    wps = _cached(cache, ('split', w.data_ptr(), w._version, bool(transposed)), w,
                  lambda: ops.pack_split_weights_dev(w.detach(), cout, cin_w, transposed=not transposed))
    ones, zeros = _ones_zeros(ops.cout_padded(cin_w), dev)
    return ops.conv_split(du.contiguous(), wps, ones, zeros, cin_w, relu=False, pool=1)
  duc = _pad_channels(du)
  cd = duc.shape[3]
  pm = _pad_map(cout, cd, dev)
  if rows is not None and n > WIDE_COUT:  # the wide node's alone; the filter read with rows and columns swapped: cout input rows, n output columns
    wpb = _cached(cache, ('wide-dgrad', w.data_ptr(), w._version, first, n), w,
                  lambda: ops.pack_wide_weights_dev(w.detach(), cin_kernel=cd, chan_map=pm, transposed=not transposed, co_first=first, co_count=n))
    ones, zeros = _ones_zeros(n, dev)
    dxr = ops.conv_wide(duc, wpb, ones, zeros, n, relu=False, pool=1)
  else:
    if first == 0 and n == cin_w:
      ws = w.contiguous()
    else:
      ws = (w.detach()[:, :, :, first:first + n] if transposed else w.detach()[:, :, first:first + n, :]).contiguous()
    wpb = _pack_dev(ws, cout, n, cd, pm, not transposed, cache, ksize=ksize)
    ones, zeros = _ones_zeros(ops.cout_padded(n), dev)
    if stored:
      assert ksize == 3 and (cout % 4 == 0 or du.dtype == torch.float32)  # bf16 du exists only behind the float4 BatchNorm kernels
      sflags = (1 if du.dtype == torch.bfloat16 else 0) | (2 if out_dtype == torch.bfloat16 else 0)
      dxr = ops.conv3x3_train(duc, wpb, ones, zeros, n, out=torch.empty((B, H, W, n), dtype=out_dtype, device=dev), store_flags=sflags,
                              moments=False)[0]
    elif ksize == 3:
      dxr = ops.conv3x3(duc, wpb, ones, zeros, n, relu=False, pool=1, bf16=bf16)
    else:
      dxr = ops.conv2d_fused(duc, wpb, ones, zeros, n, ksize, relu=False, pool=1)
  # ---- the transposed conv's stride.  It reads x[i] at dx[i] = sum_k du[2i + k - pad_lo] w[k], pad_lo = max(k - 2, 0) // 2: a
  # centred window at the ODD position 2i + 1 for k = 3, 5, 7, the EVEN position 2i itself for k = 1.  Whole pixels move, so a
  # bf16 tensor goes through the float32 kernel as channel pairs.
  if stride == 2:
    sub = _f(B, Hs, Ws, n, device=dev) if out_dtype == torch.float32 else torch.empty((B, Hs, Ws, n), dtype=out_dtype, device=dev)
    pairs = (lambda t: t.view(torch.float32)) if out_dtype == torch.bfloat16 else (lambda t: t)
    ops.subsample(pairs(dxr), even=(ksize == 1), out=pairs(sub))
    dxr = sub
  # ---- back to the kernel input's channels
  if chan_map is not None:
    dx = torch.zeros((B, Hs, Ws, Cx), dtype=out_dtype, device=dev)
    for c, j in enumerate(chan_map):
      if j >= 0:
        dx[..., c] = dxr[..., j]
    return dx
  if Cx != n:
    dx = torch.zeros((B, Hs, Ws, Cx), dtype=out_dtype, device=dev)
    dx[..., :n] = dxr
    return dx
  return dxr


class ConvBNActPool(torch.autograd.Function):
  """One layer of nnlib.cnn (nnlib.py:229-253) or nnlib.dcnn (nnlib.py:362-400) in training mode.

  x [B,Hs,Ws,Cx] (Cx % 4 == 0), w in the reference layout ([3,3,Cin,Cout]; transposed:
  [3,3,Cout,Cin]), b [Cout], gamma / beta [Cout] or None.  Returns (y, batch mean, batch var).
  A filter of size 1, 5 or 7 (meta['ksize'], default w.shape[0]) runs in float32 on ra_convkxk_f32, the two-pass batch moments
  and ra_convkxk_wgrad_f32 / _acc_f32 (csrc/ra_wgrad_kxk.hip); its filter gradient is never deferred.
  meta: transposed, stride, pool, relu, chan_map; optional: cache, bf16, sync_bn, stat_out, grads = (gw, gb, ggamma, gbeta) views
  of a gradient bucket the kernels add to, wgrad_defer + wgrad_key, and (the stacked step's sequential phase) alloc, bf16_store, y_f32."""

  @staticmethod
  def forward(ctx, x, w, b, gamma, beta, meta):
    ctx.set_materialize_grads(False)  # nothing differentiates mean / var: no zero tensors for their gradients
    dev = x.device
    x = x.contiguous()
    B, Hs, Ws, Cx = x.shape
    tr, stride, pool, relu = meta['transposed'], meta['stride'], meta['pool'], meta['relu']
    cout, cin_w = (w.shape[2], w.shape[3]) if tr else (w.shape[3], w.shape[2])
    cmap = meta.get('chan_map')
    cp = ops.cout_padded(cout)
    cache = meta.get('cache')
    cache = _PACK if cache is None else cache
    f = int(meta.get('ksize') or w.shape[0])  # the filter size: 3, or (train_any_filter) 1, 5, 7 on the float32 k x k kernels
    bf = bool(meta.get('bf16'))  # compute_dtype = 'bf16': bf16 operands on the bf16 MFMA, float32 sums and tensors
    if f != 3:
      if bf or meta.get('bf16_store'):
        raise rn.RecAttendError("a layer of filter size %d trains in float32 only (compute_dtype = 'bf16' is built for 3x3 filters)" % f)
      if cout > 128 or cp == 0:
        raise rn.RecAttendError('a layer of filter size %d trains with up to 128 output channels, not %d' % (f, cout))
    # ---- operands
    cmap_t = _cmap_dev(cmap, dev) if cmap is not None else _pad_map(cin_w, Cx, dev)
    wp = _pack_dev(w.contiguous(), cin_w, cout, Cx, cmap_t, tr, cache, ksize=f)
    scale = _ones_zeros(cp, dev, zeros=False)
    shift = _padded_shift(b, cout, cp, cache)
    use_bn = gamma is not None
    stats = None
    if use_bn:
      stats = meta['stat_out'] if meta.get('stat_out') is not None else (_f(cout, device=dev), _f(cout, device=dev))
    mean, var = stats if use_bn else (None, None)
    alloc = meta.get('alloc')  # the batched-backward step keeps u / y of a layer's T calls in one [T, ...] slab
    place = alloc if alloc is not None else (lambda kind, shape, dtype: _f(*shape, device=dev))
    up = 2 if stride == 2 else 1
    H, W = Hs * up, Ws * up
    stored = bool(meta.get('bf16_store') and alloc is not None and use_bn and not meta.get('sync_bn'))
    ud = yd = torch.float32
    if stored:
      # bf16 mode, stacked step: u and y live in HBM as bf16 where the float4 BatchNorm kernels take the channel count (else
      # float32; y also float32 where a float32 kernel reads it next: meta['y_f32']); the statistics come from the conv's
      # float32 accumulators, before the rounding.  Forward only: the stacked graph's nodes hold the backward.
      assert bf and not torch.is_grad_enabled()
      st_ok = EPILOGUE_MOMENTS['on'] and ops.bn_form('forward', cout, B, H, W, pool) == 'v4' == ops.bn_form('backward', cout, B, H, W, pool, G=1)
      ud = torch.bfloat16 if st_ok else torch.float32
      yd = torch.bfloat16 if (st_ok and not meta.get('y_f32')) else torch.float32
    # ---- conv with the batch moments
    u = _conv_moments(x, wp, scale, shift, cout, place('u', (B, H, W, cout), ud), stride, ksize=f, bf16=bf, stats=stats, stored=stored)
    # whole-batch statistics under data parallelism (nnlib.py:98): one all_gather of (count, mean, var)
    ctx.n_total = COLLECTIVES['sync_moments'](mean, var, B * H * W) if use_bn and meta.get('sync_bn') else 0.0
    # ---- normalise
    y = ops.bn_act_pool(u, mean, var, gamma, beta, relu=relu, pool=pool, out=place('y', (B, H // pool, W // pool, cout), yd),
                        store_flags=((1 if st_ok else 0) | (2 if yd == torch.bfloat16 else 0)) if stored else None)
    if stored:
      return y, mean, var
    ctx.meta, ctx.cmap, ctx.cache, ctx.ksize = meta, cmap, cache, f
    ctx.save_for_backward(x, w, u, mean, var, gamma, beta)
    if use_bn:
      ctx.mark_non_differentiable(mean, var)
      return y, mean, var
    z = torch.zeros(0, device=dev)
    ctx.mark_non_differentiable(z)
    return y, z, z

  @staticmethod
  def backward(ctx, dy, _dm, _dv):
    if dy is None:
      return None, None, None, None, None, None
    x, w, u, mean, var, gamma, beta = ctx.saved_tensors
    meta, cmap, f = ctx.meta, ctx.cmap, ctx.ksize
    dev = x.device
    tr, stride, pool, relu = meta['transposed'], meta['stride'], meta['pool'], meta['relu']
    B, Hs, Ws, Cx = x.shape
    _, H, W, cout = u.shape
    cin_w = w.shape[3] if tr else w.shape[2]
    bf = bool(meta.get('bf16'))
    grads = meta.get('grads')  # (gw, gb, ggamma, gbeta): views of the flat gradient bucket -> accumulate in-kernel
    # ---- BatchNorm / ReLU / pool
    acc = tuple(grads[2:]) if grads is not None and grads[2] is not None else None
    du, dgamma, dbeta = _bn_backward(u, dy.contiguous(), mean, var, gamma, beta, relu, pool, acc, n_total=ctx.n_total)
    # ---- the filter gradient of the SAME conv that ran, and the bias gradient
    if grads is not None:
      gw, gb = grads[:2]
      if cmap is not None:
        real = [j for j in cmap if j >= 0]
        assert len(set(real)) == len(real), 'chan_map must be injective (one writer per gradient element)'
      cmap_t = _cmap_dev(cmap, dev)
      if meta.get('wgrad_defer') is not None and f == 3:
        # the filter is shared by the step's timesteps: the end-of-backward callback reduces each layer ONCE (3x3 only: the
        # pointer-table form; another size accumulates per call)
        shape = (Cx, cout, B, Hs, Ws, H, W, int(stride == 2), tuple(cmap) if cmap is not None else None, int(cin_w), int(tr), bf)
        meta['wgrad_defer'].add(meta['wgrad_key'], x, du, shape, cmap_t, gw, gb)
      elif f != 3:
        ops.wgrad_kxk_acc(x, du, f, gw, gb, chan_map=cmap_t, transposed=tr, upsample=(stride == 2))
      else:
        ops.wgrad3x3_acc(x, du, gw, gb, chan_map=cmap_t, transposed=tr, upsample=(stride == 2), bf16=bf)
      dw = db = dgamma = dbeta = None
    else:
      dw, db = _wgrad_fresh(x, du, f, stride, bf, cmap, cin_w, tr)
    # ---- the data gradient
    dx = conv_dgrad(du, w, tr, stride, x.shape, ksize=f, chan_map=cmap, cache=ctx.cache, bf16=bf) if ctx.needs_input_grad[0] else None
    use_bn = gamma is not None
    return dx, dw, db, (dgamma if use_bn else None), (dbeta if use_bn else None), None


class BatchNormTrain(torch.autograd.Function):
  """nnlib.batch_norm with phase_train = True as an operator of its own (nnlib.py:98-119): tf.nn.moments over (B, H, W),
  gamma (x - mean) rsqrt(var + 1e-3) + beta, the batch statistics differentiated through.  x [B,H,W,C] float32.
  Returns (normed, batch mean, batch var); inside nnlib.cnn / dcnn the same kernels run fused behind the conv
  (ConvBNActPool)."""

  @staticmethod
  def forward(ctx, x, gamma, beta):
    ctx.set_materialize_grads(False)
    x = x.contiguous()
    mean, var = ops.bn_moments(x)
    y = ops.bn_act_pool(x, mean, var, gamma, beta, relu=False, pool=1)
    ctx.save_for_backward(x, mean, var, gamma, beta)
    ctx.mark_non_differentiable(mean, var)
    return y, mean, var

  @staticmethod
  def backward(ctx, dy, _dm, _dv):
    if dy is None:
      return None, None, None
    x, mean, var, gamma, beta = ctx.saved_tensors
    return ops.bn_act_pool_bwd(x, dy.contiguous(), mean, var, gamma, beta, relu=False, pool=1)


def stack_bn_reduce(info, U, dY):
  """Synchronised BatchNorm under the stacked backward, first half: the per-channel sums (sum dv, sum dv * xhat) of every
  timestep group of this rank's shard -> [G, 2 cout]; this rank's own sums also go to the gradient bucket (gamma / beta:
  the bucket all-reduce sums them over the ranks later)."""
  G, B = info['G'], info['B']
  cout = U.shape[3]
  ws = ops.bn_workspace(cout, U)
  sums = _f(G, 2 * cout, device=U.device)
  for g, (mean, var, gamma, beta, gg, gbt) in enumerate(info['per_group']):
    sl = slice(g * B, (g + 1) * B)
    ops.bn_act_pool_bwd_reduce(U[sl], dY[sl], mean, var, gamma, beta, relu=info['relu'], pool=info['pool'], acc=(gg, gbt), ws=ws,
                               out=(sums[g, :cout], sums[g, cout:]))
  return sums


def stack_bn_dx(info, U, dY, sums, n_total):
  """... second half: du of every group from the sums of the WHOLE data-parallel batch (n_total elements per channel)."""
  G, B = info['G'], info['B']
  cout = U.shape[3]
  du = torch.empty_like(U)
  for g, (mean, var, gamma, beta, _, _) in enumerate(info['per_group']):
    sl = slice(g * B, (g + 1) * B)
    ops.bn_act_pool_bwd_dx(U[sl], dY[sl], mean, var, gamma, beta, sums[g, :cout], sums[g, cout:], n_total, relu=info['relu'],
                           pool=info['pool'], du=du[sl])
  return du


def _stack_bn_backward(info, U, dY):
  """BatchNorm / ReLU / pool adjoint of a layer's G stacked calls -> du; gamma / beta gradients go to the bucket in the kernels."""
  G, B = info['G'], info['B']
  _, H, W, cout = U.shape
  relu, pool = info['relu'], info['pool']
  sflags = (1 if U.dtype == torch.bfloat16 else 0) | (2 if dY.dtype == torch.bfloat16 else 0)  # the bf16 mode's storage
  if info.get('sync_world', 1) > 1:
    # whole-batch BatchNorm (--sync_bn) under the stacked backward: the T groups' 2 C sums of a layer cross the ranks in
    # ONE all_reduce (21 collectives per step; the per-timestep graph issued T times as many)
    sums = stack_bn_reduce(info, U, dY)
    COLLECTIVES['allreduce_sums'](sums)
    return stack_bn_dx(info, U, dY, sums, float(info['sync_world']) * B * H * W)
  if sflags or ops.bn_form('backward', cout, B, H, W, pool, sflags, G=G) in ('v4', 'small'):
    # ('small': the one-channel output layer, one workgroup per timestep of the same launch; bf16 storage exists only where
    # the forward found both forms 'v4', so a refusal under it is an error)
    return ops.bn_act_pool_bwd_grouped(U, dY, info['tabs'], G, relu=relu, pool=pool, store_flags=sflags)[0]
  # no grouped form at this channel count or size (C / 4 not a power of two, e.g. the KITTI architecture's 96-channel layer;
  # a one-channel layer above the one-workgroup limit): one call per timestep
  du = torch.empty_like(U)
  ws = ops.bn_workspace(cout, U)
  for g, (mean, var, gamma, beta, gg, gbt) in enumerate(info['per_group']):
    sl = slice(g * B, (g + 1) * B)
    ops.bn_act_pool_bwd(U[sl], dY[sl], mean, var, gamma, beta, relu=relu, pool=pool, acc=(gg, gbt), ws=ws, du=du[sl])
  return du


class ConvStackFn(torch.autograd.Function):
  """The T calls of one conv + BatchNorm + ReLU + pool layer of a training step (its T timesteps: shared filter,
  per-timestep statistics and BatchNorm parameters, nnlib.py:121-127) as ONE node of the autograd graph.

  The timesteps of full_model are coupled only through the canvas, whose gradient is stopped (full_model.py:843-848),
  and the controller state starts from zero in each: once the sequential forward has filled the layer's [T, ...] slabs
  (x, u, y, statistics), the backward passes of the T timesteps are independent and run here stacked along the batch —
  one grouped BatchNorm backward (ra_bn_act_pool_bwd_grouped_f32), one filter gradient and one data gradient over
  T * B images instead of T of each.  forward() returns the precomputed y slab."""

  @staticmethod
  def forward(ctx, X, w, b, info):
    ctx.set_materialize_grads(False)
    ctx.info = info
    ctx.save_for_backward(X, w)
    return info['Y']

  @staticmethod
  def backward(ctx, dY):
    if dY is None:
      return None, None, None, None
    X, w = ctx.saved_tensors
    info = ctx.info
    U, dev = info['U'], X.device
    tr, stride, cmap, bf = info['transposed'], info['stride'], info['chan_map'], info['bf16']
    N, H, W, cout = U.shape
    du = _stack_bn_backward(info, U, dY.contiguous())
    nws = ops.wgrad3x3_workspace_floats(X.shape[3], cout, N, H, W)  # one workspace per size and step: a captured step bakes its address
    wws = _cached(info['cache'], ('wgrad_ws', nws), None, lambda: _f(nws, device=dev))
    ops.wgrad3x3_acc(X, du, info['gw'], info['gb'], chan_map=_cmap_dev(cmap, dev), transposed=tr, upsample=(stride == 2), bf16=bf, ws=wws)
    dx = None
    if ctx.needs_input_grad[0]:
      dx = conv_dgrad(du, w, tr, stride, X.shape, chan_map=cmap, cache=info['cache'], bf16=bf, out_dtype=X.dtype, allow_split=True)
    return dx, None, None, None


class WideConvBNActPool(torch.autograd.Function):
  """ConvBNActPool's contract for a layer of nnlib.cnn (nnlib.py:229-253) or nnlib.dcnn (nnlib.py:362-400) beyond K1's
  128 channels, on either side, in training mode.  float32.

  x0 [B,Hs,Ws,C0] the previous map and x1 [B,Hs,Ws,C1] the skip map or None (each % 4; concat(x0, x1) is never formed), w in the
  reference layout ([3,3,Cin,Cout]; transposed: [3,3,Cout,Cin]) whose input rows are meta['c0'] of x0's channels followed by
  meta['c1'] of x1's, b [Cout], gamma / beta [Cout] or None.  meta: transposed, stride, pool, relu, c0, c1, cache, and grads =
  (gw, gb, ggamma, gbeta) views of a gradient bucket, which then receive the parameter gradients inside the kernels.
  Returns (y, batch mean, batch var); backward returns a gradient per source.  A constant number of launches per layer:
    Cout > 128   K1-wide, ra_bn_wide_*, ra_conv3x3_wgrad_wide_acc_f32 (once per source, through a channel map)
    Cout <= 128  K1, ra_bn_*, ra_conv3x3_wgrad_acc_f32 (likewise): only the data gradient is wide
  and the data gradient per source by conv_dgrad on that source's rows of the filter."""

  @staticmethod
  def forward(ctx, x0, x1, w, b, gamma, beta, meta):
    ctx.set_materialize_grads(False)
    dev = x0.device
    x0 = x0.contiguous()
    x1 = None if x1 is None else x1.contiguous()
    B, Hs, Ws, C0 = x0.shape
    C1 = 0 if x1 is None else x1.shape[3]
    tr, stride, pool, relu = meta['transposed'], meta['stride'], meta['pool'], meta['relu']
    cout, cin_w = (w.shape[2], w.shape[3]) if tr else (w.shape[3], w.shape[2])
    c0, c1 = meta['c0'], meta.get('c1', 0)
    if c0 + c1 != cin_w or c0 > C0 or c1 > C1 or tuple(w.shape[:2]) != (3, 3):
      raise rn.RecAttendError('WideConvBNActPool: a 3x3 filter of %d input rows for sources of %d (of %d) + %d (of %d) channels' %
                              (cin_w, c0, C0, c1, C1))
    cache = meta.get('cache')
    cache = _PACK if cache is None else cache
    whole, _, _ = _source_maps(c0, C0, c1, C1, dev)
    use_bn = gamma is not None
    mean = var = None
    # ---- operands, conv with the batch moments, normalise: the wide kernels beyond 128 output channels, else the narrow ones
    if cout > WIDE_COUT:
      wp = _cached(cache, ('wide', w.data_ptr(), w._version, C0, C1, bool(tr)), w,
                   lambda: ops.pack_wide_weights_dev(w.detach().contiguous(), cin_kernel=C0 + C1, chan_map=whole, transposed=tr))
      ones, _ = _ones_zeros(cout, dev)
      u = ops.conv_wide(x0, wp, ones, b.detach(), cout, relu=False, pool=1, src1=x1, upsample=(stride == 2))
      if use_bn:
        mean, var = ops.bn_wide_moments(u)
      y = ops.bn_wide_act_pool(u, mean, var, gamma, beta, relu=relu, pool=pool)
    else:
      cp = ops.cout_padded(cout)
      ones, _ = _ones_zeros(cp, dev)
      shift = b.detach() if cp == cout else torch.nn.functional.pad(b.detach(), (0, cp - cout))
      wp = _pack_dev(w.contiguous(), cin_w, cout, C0 + C1, whole, tr, cache)
      u = ops.conv3x3(x0, wp, ones, shift, cout, relu=False, pool=1, src1=x1, upsample=(stride == 2))
      if use_bn:
        mean, var = ops.bn_moments(u, out=(_f(cout, device=dev), _f(cout, device=dev)))
      y = ops.bn_act_pool(u, mean, var, gamma, beta, relu=relu, pool=pool, out=_f(B, u.shape[1] // pool, u.shape[2] // pool, cout, device=dev))
    ctx.meta, ctx.cache = meta, cache
    ctx.save_for_backward(x0, x1, w, u, mean, var, gamma, beta)
    if use_bn:
      ctx.mark_non_differentiable(mean, var)
      return y, mean, var
    z = torch.zeros(0, device=dev)
    ctx.mark_non_differentiable(z)
    return y, z, z

  @staticmethod
  def backward(ctx, dy, _dm, _dv):
    if dy is None:
      return None, None, None, None, None, None, None
    x0, x1, w, u, mean, var, gamma, beta = ctx.saved_tensors
    meta, cache = ctx.meta, ctx.cache
    dev = x0.device
    tr, stride, pool, relu = meta['transposed'], meta['stride'], meta['pool'], meta['relu']
    C0 = x0.shape[3]
    C1 = 0 if x1 is None else x1.shape[3]
    B, H, W, cout = u.shape
    c0, c1 = meta['c0'], meta.get('c1', 0)
    _, m0, m1 = _source_maps(c0, C0, c1, C1, dev)
    dy = dy.contiguous()
    grads = meta.get('grads')  # views of the flat gradient bucket: the kernels add to them; else fresh tensors are returned
    if grads is not None:
      gw, gb, gg, gbt = grads
    else:
      gw, gb, gg, gbt = torch.zeros_like(w), torch.zeros(cout, dtype=torch.float32, device=dev), None, None
    ups = stride == 2
    sources = [(xs, ms) for xs, ms in ((x0, m0), (x1, m1)) if xs is not None]
    # ---- BatchNorm / ReLU / pool, then the filter gradient of the SAME conv that ran, source by source (gb once)
    if cout > WIDE_COUT:
      du, dgamma, dbeta = ops.bn_wide_act_pool_bwd(u, dy, mean, var, gamma, beta, relu=relu, pool=pool, acc_gamma=gg, acc_beta=gbt)
      for xs, ms in sources:
        ops.wgrad_wide_acc(xs, du, gw, gb if xs is x0 else None, chan_map=ms, transposed=tr, upsample=ups)
    else:
      du, dgamma, dbeta = _bn_backward(u, dy, mean, var, gamma, beta, relu, pool, (gg, gbt))
      for xs, ms in sources:
        ops.wgrad3x3_acc(xs, du, gw, gb if xs is x0 else None, chan_map=ms, transposed=tr, upsample=ups)
    # ---- the data gradient, one conv per source on its rows of the filter
    dx = [None, None]
    if any(ctx.needs_input_grad[:2]):
      duc = _pad_channels(du)
      for s, (xs, first, n) in enumerate(((x0, 0, c0), (x1, c0, c1))):
        if xs is not None and ctx.needs_input_grad[s]:
          dx[s] = conv_dgrad(duc, w, tr, stride, tuple(xs.shape), rows=(first, n), cache=cache)
    use_bn = gamma is not None
    if grads is not None:
      return dx[0], dx[1], None, None, None, None, None
    return dx[0], dx[1], gw, gb, (dgamma if use_bn else None), (dbeta if use_bn else None), None
