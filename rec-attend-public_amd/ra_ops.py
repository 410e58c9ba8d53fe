"""Thin torch-tensor wrappers over the C ABI (include/recattend.h).

Every function here launches hand-written HIP kernels from librecattend.so on the current
torch stream.  Inputs must be float32 CUDA tensors (contiguous); there is no CPU path —
calling with CPU tensors raises.  Host-side weight repacking (ra_conv_pack_weights,
ra_conv_fold_bn, ra_ctrl_pack_weights) runs in the library's C++ and works without a GPU.
"""
import ctypes as C
import os

import numpy as np
import torch

import ra_native as rn
from ra_native import check, ptr

BN_EPS = 1e-3  # nnlib.py:119


def _need_cuda(*ts, f32=True):
  """f32=False: tensors that may be stored as bf16 (checked for device and contiguity only)."""
  for t in ts:
    if t is not None and not t.is_cuda:
      raise rn.RecAttendError('recattend kernels need CUDA (HIP) tensors; got a CPU tensor. '
                              'There is no CPU fallback.')
    if t is not None and ((f32 and t.dtype != torch.float32) or not t.is_contiguous()):
      raise rn.RecAttendError('recattend kernels need contiguous float32 tensors')


def _np32(a):
  if isinstance(a, torch.Tensor):
    a = a.detach().cpu().numpy()
  return np.ascontiguousarray(a, dtype=np.float32)


# ---------------------------------------------------------------------------- host packing


def cout_padded(cout):
  return rn.lib().ra_conv_cout_padded(int(cout))


FILTER_SIZES = (1, 3, 5, 7)  # the K1 filter sizes built (ra_convkxk_f32)


def _filter_channels(w, cin_kernel, chan_map, transposed):
  """(cin_w, cout, cin, chan_map, flags) of a filter w [f,f,Ci,Co] (transposed: [f,f,Co,Ci]) for a kernel input of cin_kernel
  channels: what pack_conv_weights and pack_wide_weights hand to their pack entry points."""
  cin_w, cout = (w.shape[3], w.shape[2]) if transposed else (w.shape[2], w.shape[3])
  cin = cin_w if cin_kernel is None else int(cin_kernel)
  if chan_map is None and cin != cin_w:
    chan_map = list(range(cin_w)) + [-1] * (cin - cin_w)
  return cin_w, cout, cin, chan_map, rn.RA_CONV_TRANSPOSED if transposed else 0


def _chan_map_i32(chan_map, cin):
  if chan_map is None:
    return None
  cm = np.ascontiguousarray(chan_map, dtype=np.int32)
  assert cm.shape[0] == cin
  return cm


def pack_conv_weights(w, cin_kernel=None, chan_map=None, transposed=False):
  """TF-layout filter -> packed B-operand order (numpy, host).  w [f,f,Ci,Co] or, when
  transposed, the conv2d_transpose filter [f,f,Co,Ci]; f in FILTER_SIZES (3: ra_conv_pack_weights,
  else ra_conv_pack_weights_k — the input of conv2d_fused(..., ksize=f))."""
  w = _np32(w)
  f = w.shape[0]
  if w.ndim != 4 or w.shape[1] != f or f not in FILTER_SIZES:
    raise rn.RecAttendError('filter of shape %r: square filters of size %s are built' % (w.shape, FILTER_SIZES))
  cin_w, cout, cin, chan_map, flags = _filter_channels(w, cin_kernel, chan_map, transposed)
  if cout > 128 and f == 3 and conv_wide_supported(cin, cout):  # the wide layer's own order (conv_wide / conv2d_fused run it)
    return pack_wide_weights(w, cin_kernel=cin, chan_map=chan_map, transposed=transposed)
  if cout > 128 and f != 3 and conv_wide_supported(cin, cout):
    raise rn.RecAttendError('wide layers (Cout = %d > 128) are built for 3x3 filters only, not %dx%d' % (cout, f, f))
  n = rn.lib().ra_conv_packed_floats(cin, cout) if f == 3 else rn.lib().ra_conv_packed_floats_k(f, cin, cout)
  if n == 0:
    raise rn.RecAttendError('unsupported conv shape Cin=%d Cout=%d' % (cin, cout))
  out = np.empty(n, dtype=np.float32)
  cm = _chan_map_i32(chan_map, cin)
  if f == 3:
    check(rn.lib().ra_conv_pack_weights(ptr(w), cin_w, cout, cin, ptr(cm), flags, ptr(out)), 'ra_conv_pack_weights')
  else:
    check(rn.lib().ra_conv_pack_weights_k(ptr(w), f, cin_w, cout, cin, ptr(cm), flags, ptr(out)), 'ra_conv_pack_weights_k')
  return out


def fold_bn(bias, cout, bn=None):
  """(scale, shift) [CoutP] numpy.  bn = (beta, gamma, ema_mean, ema_var) or None."""
  cp = cout_padded(cout)
  if cp == 0 and 128 < cout <= 512:  # a wide layer (conv_wide): Cout floats each, the same float32 fold as ra_conv_fold_bn
    b = np.zeros(cout, np.float32) if bias is None else _np32(bias)
    if bn is None:
      return np.ones(cout, np.float32), b.copy()
    beta, gamma, mean, var = (_np32(a) for a in bn)
    sc = (gamma / np.sqrt(var + np.float32(BN_EPS))).astype(np.float32)
    return sc, ((b - mean) * sc + beta).astype(np.float32)
  scale = np.empty(cp, dtype=np.float32)
  shift = np.empty(cp, dtype=np.float32)
  b = None if bias is None else _np32(bias)
  if bn is None:
    args = (None, None, None, None)
  else:
    args = tuple(_np32(a) for a in bn)
  keep = (b,) + args
  check(rn.lib().ra_conv_fold_bn(ptr(b), ptr(args[0]), ptr(args[1]), ptr(args[2]), ptr(args[3]),
                                 int(cout), C.c_float(BN_EPS), ptr(scale), ptr(shift)),
        'ra_conv_fold_bn')
  del keep
  return scale, shift


def make_ctrl_desc(G, Cf, hid, iters, n_gmlp, n_cmlp, mlp_dim, H, W, Fh, Fw, squash, fixed_var,
                   dynamic_var, fixed_gamma):
  return rn.CtrlDesc(int(G), int(Cf), int(hid), int(iters), int(n_gmlp), int(n_cmlp),
                     int(mlp_dim), int(H), int(W), int(Fh), int(Fw), int(bool(squash)),
                     int(bool(fixed_var)), int(bool(dynamic_var)), int(bool(fixed_gamma)))


def _pack_ctrl(desc, lstm, gmlp, cmlp, count_fn, pack_fn, unsupported):
  """The controller's weights in the order of the library's pack_fn, count_fn floats of them (numpy, host)."""
  n = getattr(rn.lib(), count_fn)(C.byref(desc))
  if n == 0:
    raise rn.RecAttendError(unsupported)
  order = ['w_xi', 'w_hi', 'b_i', 'w_xf', 'w_hf', 'b_f', 'w_xu', 'w_hu', 'b_u', 'w_xo', 'w_ho',
           'b_o']
  la = [_np32(lstm[k]) for k in order]
  ga = [_np32(a) for wb in gmlp for a in wb]
  ca = [_np32(a) for wb in cmlp for a in wb]
  arr = lambda xs: (C.c_void_p * len(xs))(*[x.ctypes.data for x in xs])
  out = np.empty(n, dtype=np.float32)
  check(getattr(rn.lib(), pack_fn)(C.byref(desc), arr(la), arr(ga), arr(ca), ptr(out)), pack_fn)
  return out


def pack_ctrl_weights(desc, lstm, gmlp, cmlp):
  """lstm: dict with keys w_xi,w_hi,b_i,...; gmlp/cmlp: lists [(w,b),...].  -> numpy."""
  return _pack_ctrl(desc, lstm, gmlp, cmlp, 'ra_ctrl_packed_floats', 'ra_ctrl_pack_weights', 'unsupported controller descriptor')


def ctrl_split_supported(desc):
  return bool(rn.lib().ra_ctrl_split_supported(C.byref(desc)))


def pack_ctrl_split_weights(desc, lstm, gmlp, cmlp):
  return _pack_ctrl(desc, lstm, gmlp, cmlp, 'ra_ctrl_split_packed_floats', 'ra_ctrl_split_pack_weights',
                    'descriptor not supported by the split controller')


_CUS = []


def cu_count():
  """Compute units of the current device (256 on MI355X)."""
  if not _CUS:
    _CUS.append(int(torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count))
  return _CUS[0]


def _exchange_workspace(desc, B, device, bytes_fn):
  nb = getattr(rn.lib(), bytes_fn)(C.byref(desc), B)
  return (torch.zeros((nb + 7) // 8, dtype=torch.int64, device=device),
          torch.zeros(1, dtype=torch.int32, device=device))


def ctrl_split_workspace(desc, B, device):
  """Zero-filled exchange workspace (+ status word) for ONE stream of launches."""
  return _exchange_workspace(desc, B, device, 'ra_ctrl_split_workspace_bytes')


def controller_split(desc, feat, wp, h_last, ctrl_out, gmaps, attn, ws, status):
  _need_cuda(feat, wp, h_last, ctrl_out, gmaps, attn)
  check(rn.lib().ra_controller_split_f32(C.byref(desc), ptr(feat), ptr(wp), feat.shape[0],
                                         ptr(h_last), ptr(ctrl_out), ptr(gmaps), ptr(attn),
                                         ptr(ws), ws.numel() * 8, ptr(status), rn.stream_ptr()),
        'ra_controller_split_f32')


def ctrl_batch_group(desc, B):
  """Images that share one set of 16 controller workgroups in a controller_batch (K2b) launch of B images."""
  return int(rn.lib().ra_ctrl_batch_group_images(C.byref(desc), int(B)))


def ctrl_batch_supported(desc):
  return bool(rn.lib().ra_ctrl_batch_supported(C.byref(desc)))


def ctrl_batch_workspace(desc, B, device):
  """Zero-filled exchange workspace (+ status word) of the group-shared controller, for ONE stream of launches."""
  return _exchange_workspace(desc, B, device, 'ra_ctrl_batch_workspace_bytes')


def ctrl_form(desc, B, co_resident=1, cus=None):
  """The controller form a launch of B images runs beside co_resident - 1 launches of its kind on a device of cus compute
  units (default: the current device's): 'split' (16 workgroups per image), 'batch' (16 per group of ctrl_batch_group
  images) or None (the one-workgroup kernel).  The workgroups of a team exchange through spin-waits, so ALL workgroups of
  every launch that can be running at the same time must be resident at once (112 KB of LDS each: one per CU), with a
  margin of 32 CUs for everything else: 224 of the MI355X's 256, the bound the C entry points check per launch."""
  if not ctrl_split_supported(desc):
    return None
  room = (cu_count() if cus is None else int(cus)) - 32
  n = 16 * max(1, int(co_resident))
  if B * n <= room:
    return 'split'
  if ctrl_batch_supported(desc) and -(-B // ctrl_batch_group(desc, B)) * n <= room:
    return 'batch'  # more than 14 images, or launches that overlap
  return None


_BN_PASSES = {'moments': rn.RA_BN_PASS_MOMENTS, 'forward': rn.RA_BN_PASS_FORWARD, 'backward': rn.RA_BN_PASS_BACKWARD}
_BN_FORMS = {rn.RA_BN_FORM_SMALL: 'small', rn.RA_BN_FORM_V4: 'v4', rn.RA_BN_FORM_GENERIC: 'generic'}


def bn_form(which, C, B, H, W, pool=1, flags=0, stages=3, G=0):
  """The kernel form the BatchNorm pass `which` ('moments', 'forward', 'backward') runs over u [B,H,W,C]: 'small' (one
  workgroup), 'v4' (four channels per thread: the only form with bf16 storage, flags != 0) or 'generic', or the negative
  RA_E_* code with which the entry point refuses the call (ra_bn_form: the library's own chooser, no launch).  stages: of a
  per-call backward (1 = reduce, 2 = dx, 3 = one call); G > 0: the grouped backward over G groups."""
  rc = rn.lib().ra_bn_form(_BN_PASSES[which], int(C), int(B), int(H), int(W), int(pool), int(flags), int(stages), int(G))
  return _BN_FORMS.get(rc, rc)


def controller_batch(desc, feat, wp, h_last, ctrl_out, gmaps, attn, ws, status, xcd_offset=-1):
  """K2b: ra_controller_split_f32's recurrence with the weight slices shared by groups of ctrl_batch_group(desc, B) images.
  xcd_offset >= 0: the XCD-local exchange, group g on XCD (g + xcd_offset) % 8 (ra_controller_batch_xcd_f32: the caller keeps
  concurrent launches on different XCDs); -1: agent-scope atomics."""
  _need_cuda(feat, wp, h_last, ctrl_out, gmaps, attn)
  check(rn.lib().ra_controller_batch_xcd_f32(C.byref(desc), ptr(feat), ptr(wp), feat.shape[0], ptr(h_last), ptr(ctrl_out),
                                             ptr(gmaps), ptr(attn), ptr(ws), ws.numel() * 8, ptr(status), int(xcd_offset), rn.stream_ptr()),
        'ra_controller_batch_xcd_f32')


# ---------------------------------------------------------------------------- device ops


def _conv_out(src, cout, pool=1, upsample=False, out=None, checked_for=None):
  """The output [B,Ho,Wo,cout] of a conv layer over src [B,Hs,Ws,.]: Ho, Wo = Hs, Ws (twice that with upsample) // pool.
  A fresh tensor when out is None; checked_for: the wrapper that has a given out's shape checked."""
  B, Hs, Ws = src.shape[:3]
  up = 2 if upsample else 1
  shape = (B, Hs * up // pool, Ws * up // pool, cout)
  if out is None:
    return torch.empty(shape, dtype=torch.float32, device=src.device)
  if checked_for and tuple(out.shape) != shape:
    raise rn.RecAttendError('%s: out of shape %r, expected %r' % (checked_for, tuple(out.shape), shape))
  return out


def conv3x3(src0, wp, scale, shift, cout, relu=True, pool=1, src1=None, upsample=False,
            out=None, plane=None, plane_chan=-1, bf16=False):
  """One fused conv layer.  src0 [B,Hs,Ws,C0] (+ src1 [B,Hs,Ws,C1]) -> [B,Ho,Wo,cout].
  bf16: bf16 operands on the bf16 MFMA, float32 accumulation (the training step's mixed-precision mode)."""
  _need_cuda(src0, src1, wp, scale, shift, out)
  B, Hs, Ws, C0 = src0.shape
  C1 = 0 if src1 is None else src1.shape[3]
  out = _conv_out(src0, cout, pool, upsample, out)
  fn = rn.lib().ra_conv3x3_bf16ops_f32 if bf16 else rn.lib().ra_conv3x3_f32
  check(fn(ptr(src0), C0, ptr(src1), C1, B, Hs, Ws, int(upsample), ptr(wp), ptr(scale), ptr(shift), int(cout),
           int(relu), int(pool), ptr(plane), int(plane_chan), ptr(out), rn.stream_ptr()),
        'ra_conv3x3_bf16ops_f32' if bf16 else 'ra_conv3x3_f32')
  return out


# ---- launch plans (recattend.h, RA_PLAN_*): which template instantiation, grid and tile walk a conv entry point would launch
_PLAN_FAMILIES = {v: k[len('RA_PLAN_FAMILY_'):].lower() for k, v in rn.CONSTANTS.items() if k.startswith('RA_PLAN_FAMILY_')}
_PLAN_FORMS = sorted((v, k[len('RA_PLAN_FORM_'):].lower()) for k, v in rn.CONSTANTS.items() if k.startswith('RA_PLAN_FORM_'))
_PLAN_FIELDS = sorted((v, k[len('RA_PLAN_'):].lower()) for k, v in rn.CONSTANTS.items()
                      if k.startswith('RA_PLAN_') and not k.startswith(('RA_PLAN_FAMILY_', 'RA_PLAN_FORM_')) and k != 'RA_PLAN_INTS')


def plan_dict(rec):
  """A plan record (the RA_PLAN_INTS ints a ra_*_plan query fills) as a dict: 'family' by name, 'form' as the sorted tuple
  of its bits' names, every other RA_PLAN_* field as an int."""
  out = {field: rec[i] for i, field in _PLAN_FIELDS}
  out['family'] = _PLAN_FAMILIES[rec[rn.RA_PLAN_FAMILY]]
  out['form'] = tuple(sorted(n for bit, n in _PLAN_FORMS if rec[rn.RA_PLAN_FORM] & bit))
  return out


def _plan(name, *args):
  """plan_dict of the record the query `name` fills.  Host only: nothing is launched."""
  rec = (C.c_int * rn.RA_PLAN_INTS)()
  check(getattr(rn.lib(), name)(*([int(a) for a in args] + [rec])), name)
  return plan_dict(rec)


def conv3x3_plan(c0, c1, B, Hs, Ws, cout, pool=1, upsample=False, ksize=3, plane=False, bf16=False, moments=False, store_flags=0):
  """Plan of conv3x3 / conv2d_fused (ksize) / the bf16-operand and moments entry points on these shape arguments.  Needs no
  device; without one grid, tiles_min and tiles_max are -1."""
  return _plan('ra_conv3x3_plan', c0, c1, B, Hs, Ws, bool(upsample), ksize, cout, pool, bool(plane), bool(bf16), bool(moments), store_flags)


def conv_pair_plan(cin, B, Hs, Ws, couta, coutb, poolB=2, upsampleA=False, plane=False, cache_form=0):
  """Plan of conv_pair (cache_form 0), conv_pair_fill_cache (1) or conv_pair_cached (2).  The geometry and the N-packed
  kernel's plan need no device; whether the persistent kernel runs does (grid -1 without one)."""
  return _plan('ra_conv_pair_plan', cin, B, Hs, Ws, bool(upsampleA), couta, coutb, poolB, bool(plane), cache_form)


def conv_split_plan(B, H, W, cin, cout, pool=1, plane=False):
  return _plan('ra_conv_split_plan', B, H, W, cin, cout, pool, bool(plane))


def conv_wino_plan(B, H, W, cin, cout, pool=1):
  return _plan('ra_conv_wino_plan', B, H, W, cin, cout, pool)


def conv_pair_wino_plan(B, H, W):
  return _plan('ra_conv_pair_wino_plan', B, H, W)


def conv_pair16_plan(B, H, W):
  return _plan('ra_conv_pair16_plan', B, H, W)


def conv2d_fused(src0, wp, scale, shift, cout, ksize, relu=True, pool=1, src1=None, upsample=False, out=None, plane=None,
                 plane_chan=-1):
  """conv3x3 for a ksize x ksize filter, ksize in FILTER_SIZES; wp = pack_conv_weights of that filter.  ksize = 3 IS
  conv3x3; other sizes run ra_convkxk_f32 (float32 operands only)."""
  if cout > 128:  # K1 stops at 128 output channels: the wide layer (3x3 only, no canvas plane)
    if ksize != 3 or plane is not None:
      raise rn.RecAttendError('wide layers (Cout = %d > 128) are built for 3x3 filters without a canvas plane' % cout)
    return conv_wide(src0, wp, scale, shift, cout, relu=relu, pool=pool, src1=src1, upsample=upsample, out=out)
  if ksize == 3:
    return conv3x3(src0, wp, scale, shift, cout, relu=relu, pool=pool, src1=src1, upsample=upsample, out=out, plane=plane,
                   plane_chan=plane_chan)
  _need_cuda(src0, src1, wp, scale, shift, out)
  B, Hs, Ws, C0 = src0.shape
  C1 = 0 if src1 is None else src1.shape[3]
  out = _conv_out(src0, cout, pool, upsample, out)
  check(rn.lib().ra_convkxk_f32(ptr(src0), C0, ptr(src1), C1, B, Hs, Ws, int(upsample), ptr(wp), int(ksize), ptr(scale),
                                ptr(shift), int(cout), int(relu), int(pool), ptr(plane), int(plane_chan), ptr(out),
                                rn.stream_ptr()), 'ra_convkxk_f32')
  return out


# ---- training layers of filter size 1, 5 and 7 (csrc/ra_wgrad_kxk.hip; ra_layer_train.ConvBNActPool)

_WGK_FIELDS = sorted((v, k[len('RA_WGK_PLAN_'):].lower()) for k, v in rn.CONSTANTS.items() if k.startswith('RA_WGK_PLAN_') and k != 'RA_WGK_PLAN_INTS')


def wgrad_kxk_plan(ksize, cin, cout, B, H, W):
  """The launch the k x k filter gradient (ksize in 1, 5, 7) takes for a conv map [B,H,W,cout] of cin kernel channels
  (ra_convkxk_wgrad_plan: host only): {'nt', 'grid_x', 'grid_y', 'grid_z', 'lds_bytes', 'record_floats', 'ntiles', 'acc_tiles'}."""
  rec = (C.c_int * rn.RA_WGK_PLAN_INTS)()
  check(rn.lib().ra_convkxk_wgrad_plan(int(ksize), int(cin), int(cout), int(B), int(H), int(W), rec), 'ra_convkxk_wgrad_plan')
  return {name: rec[i] for i, name in _WGK_FIELDS}


def pack_conv_weights_dev(w, ksize, cin_kernel=None, chan_map=None, transposed=False):
  """pack_conv_weights of a ksize x ksize filter on the device (the weights change every step): w [k,k,Ci,Co] (transposed:
  [k,k,Co,Ci]) a device tensor, chan_map an int32 device tensor or None -> the input of conv2d_fused(..., ksize=k)."""
  _need_cuda(w)
  if w.dim() != 4 or tuple(w.shape[:2]) != (ksize, ksize):
    raise rn.RecAttendError('filter of shape %r is not %d x %d' % (tuple(w.shape), ksize, ksize))
  cin_w, cout = (w.shape[3], w.shape[2]) if transposed else (w.shape[2], w.shape[3])
  cin = cin_w if cin_kernel is None else int(cin_kernel)
  if chan_map is not None and not (chan_map.is_cuda and chan_map.dtype == torch.int32 and chan_map.numel() == cin):
    raise rn.RecAttendError('pack_conv_weights_dev: chan_map must be an int32 device tensor of %d entries' % cin)
  n = rn.lib().ra_conv_packed_floats_k(int(ksize), cin, int(cout))
  if n == 0:
    raise rn.RecAttendError('unsupported conv shape k=%d Cin=%d Cout=%d (k in 1, 3, 5, 7; Cin %% 4; Cout <= 128)' % (ksize, cin, cout))
  out = torch.empty(n, dtype=torch.float32, device=w.device)
  check(rn.lib().ra_conv_pack_weights_k_dev(ptr(w), int(ksize), int(cin_w), int(cout), cin, ptr(chan_map),
                                            rn.RA_CONV_TRANSPOSED if transposed else 0, ptr(out), rn.stream_ptr()), 'ra_conv_pack_weights_k_dev')
  return out


def _wgrad_kxk_args(who, x, du, ksize, upsample, ws):
  _need_cuda(x, du, ws)
  B, Hs, Ws, cin = x.shape
  H, W, cout = du.shape[1:]
  up = 2 if upsample else 1
  if tuple(du.shape[:3]) != (B, Hs * up, Ws * up) or not (x.is_contiguous() and du.is_contiguous()):
    raise rn.RecAttendError('%s: contiguous x of %r and du of %r' % (who, tuple(x.shape), tuple(du.shape)))
  n = rn.lib().ra_convkxk_wgrad_workspace_floats(int(ksize), cin, cout, B, H, W)
  if n == 0:
    raise rn.RecAttendError('%s: unsupported shape k=%d Cin=%d Cout=%d (k in 1, 3, 5, 7; Cin %% 4; Cout <= 128)' % (who, ksize, cin, cout))
  if ws is None or ws.numel() < n:
    ws = torch.empty(n, dtype=torch.float32, device=x.device)
  return B, Hs, Ws, cin, cout, ws


def wgrad_kxk(x, du, ksize, upsample=False, ws=None, dw=None, db=None):
  """(dw [k,k,Cin,Cout], db [Cout]) of the ksize x ksize conv that ran on x [B,Hs,Ws,Cin] (Cin % 4 == 0) and produced du's
  tensor [B,H,W,Cout], Cout <= 128; upsample: the stride-2 transposed form.  ksize = 3 is the 3x3 kernel.  ws: a workspace
  to reuse (ra_convkxk_wgrad_workspace_floats floats)."""
  B, Hs, Ws, cin, cout, ws = _wgrad_kxk_args('wgrad_kxk', x, du, ksize, upsample, ws)
  dw = torch.empty((ksize, ksize, cin, cout), dtype=torch.float32, device=x.device) if dw is None else dw
  db = torch.empty(cout, dtype=torch.float32, device=x.device) if db is None else db
  _need_cuda(dw, db)
  check(rn.lib().ra_convkxk_wgrad_f32(ptr(x), cin, B, Hs, Ws, int(bool(upsample)), ptr(du), cout, int(ksize), ptr(ws), ws.numel(), ptr(dw),
                                      ptr(db), rn.stream_ptr()), 'ra_convkxk_wgrad_f32')
  return dw, db


def wgrad_kxk_acc(x, du, ksize, gw, gb=None, chan_map=None, transposed=False, upsample=False, ws=None):
  """gw += the filter gradient of wgrad_kxk in the reference layout of the filter that ran ([k,k,cin_w,Cout]; transposed:
  [k,k,Cout,cin_w] with flipped taps), gb += the bias gradient (None: not wanted).  chan_map (int32 device tensor, or None)
  sends kernel channel c to filter row chan_map[c], -1 = padding."""
  B, Hs, Ws, cin, cout, ws = _wgrad_kxk_args('wgrad_kxk_acc', x, du, ksize, upsample, ws)
  _need_cuda(gw, gb)
  cin_w = gw.shape[3] if transposed else gw.shape[2]
  if tuple(gw.shape) != ((ksize, ksize, cout, cin_w) if transposed else (ksize, ksize, cin_w, cout)) or not gw.is_contiguous() or \
      (gb is not None and gb.numel() != cout):
    raise rn.RecAttendError('wgrad_kxk_acc: gw of %r / gb for %d output channels' % (tuple(gw.shape), cout))
  if chan_map is not None and not (chan_map.is_cuda and chan_map.dtype == torch.int32 and chan_map.numel() == cin):
    raise rn.RecAttendError('wgrad_kxk_acc: chan_map must be an int32 device tensor of %d entries' % cin)
  check(rn.lib().ra_convkxk_wgrad_acc_f32(ptr(x), cin, B, Hs, Ws, int(bool(upsample)), ptr(du), cout, int(ksize), ptr(ws), ws.numel(),
                                          ptr(chan_map), int(cin_w), int(bool(transposed)), ptr(gw), ptr(gb), rn.stream_ptr()),
        'ra_convkxk_wgrad_acc_f32')
  return gw


def conv_wide_supported(cin, cout):
  """The wide 3x3 layer takes Cout 129 .. 512 (a multiple of 16) and cin = C0 + C1 <= 1024 (a multiple of 4)."""
  return bool(rn.lib().ra_conv_wide_supported(int(cin), int(cout)))


def pack_wide_weights(w, cin_kernel=None, chan_map=None, transposed=False):
  """pack_conv_weights for the wide layer: w [3,3,Ci,Co] (transposed: [3,3,Co,Ci]) -> ra_conv_wide_pack_weights' order
  [co / 64][c / 16][tap][ksub][co % 64][cg], channel c = 16 chunk + 4 cg + ksub (numpy, host)."""
  w = _np32(w)
  if w.ndim != 4 or tuple(w.shape[:2]) != (3, 3):
    raise rn.RecAttendError('filter of shape %r: wide layers are built for 3x3 filters only' % (w.shape,))
  cin_w, cout, cin, chan_map, flags = _filter_channels(w, cin_kernel, chan_map, transposed)
  n = rn.lib().ra_conv_wide_packed_floats(cin, cout)
  if n == 0:
    raise rn.RecAttendError('unsupported wide conv shape Cin=%d Cout=%d (Cin %% 4, <= 1024; Cout 129 .. 512, %% 16)' % (cin, cout))
  out = np.empty(n, dtype=np.float32)
  cm = _chan_map_i32(chan_map, cin)
  check(rn.lib().ra_conv_wide_pack_weights(ptr(w), cin_w, cout, cin, ptr(cm), flags, ptr(out)), 'ra_conv_wide_pack_weights')
  return out


def conv_wide(src0, wp, scale, shift, cout, relu=True, pool=1, src1=None, upsample=False, out=None):
  """conv3x3 for Cout 129 .. 512: src0 [B,Hs,Ws,C0] (+ src1 [B,Hs,Ws,C1]) -> [B,Ho,Wo,cout]; wp = pack_wide_weights,
  scale / shift of cout floats (fold_bn)."""
  _need_cuda(src0, src1, wp, scale, shift, out)
  B, Hs, Ws, C0 = src0.shape
  C1 = 0 if src1 is None else src1.shape[3]
  if src1 is not None and tuple(src1.shape[:3]) != (B, Hs, Ws):
    raise rn.RecAttendError('conv_wide: sources of %r and %r' % (tuple(src0.shape), tuple(src1.shape)))
  n = rn.lib().ra_conv_wide_packed_floats(C0 + C1, int(cout))
  if n == 0 or wp.numel() != n or scale.numel() < cout or shift.numel() < cout:
    raise rn.RecAttendError('conv_wide: unsupported shape Cin=%d Cout=%d, or weights not packed for it' % (C0 + C1, cout))
  out = _conv_out(src0, cout, pool, upsample, out, checked_for='conv_wide')
  check(rn.lib().ra_conv3x3_wide_f32(ptr(src0), C0, ptr(src1), C1, B, Hs, Ws, int(upsample), ptr(wp), ptr(scale), ptr(shift),
                                     int(cout), int(relu), int(pool), ptr(out), rn.stream_ptr()), 'ra_conv3x3_wide_f32')
  return out


# ---- training the wide layers (csrc/ra_wgrad_wide.hip, ra_bn_wide.hip; ra_layer_train.WideConvBNActPool)


def pack_wide_weights_dev(w, cin_kernel=None, chan_map=None, transposed=False, co_first=0, co_count=None):
  """pack_wide_weights on the device (the weights change every step), for the output channels [co_first, co_first + co_count)
  of the filter: w [3,3,Ci,Co] (transposed: [3,3,Co,Ci]) a device tensor, chan_map an int32 device tensor or None -> the
  packed slice, bit-equal to the host pack of w's slice.  With `transposed` toggled and Ci / Co swapped by the caller it is the
  data gradient's packing."""
  _need_cuda(w)
  if w.dim() != 4 or tuple(w.shape[:2]) != (3, 3):
    raise rn.RecAttendError('filter of shape %r: wide layers are built for 3x3 filters only' % (tuple(w.shape),))
  cin_w, cout = (w.shape[3], w.shape[2]) if transposed else (w.shape[2], w.shape[3])
  cin = cin_w if cin_kernel is None else int(cin_kernel)
  co_count = cout - co_first if co_count is None else int(co_count)
  if chan_map is None and cin != cin_w:
    raise rn.RecAttendError('pack_wide_weights_dev: a kernel input of %d channels for %d filter rows needs a chan_map' % (cin, cin_w))
  if chan_map is not None and not (chan_map.is_cuda and chan_map.dtype == torch.int32 and chan_map.numel() == cin):
    raise rn.RecAttendError('pack_wide_weights_dev: chan_map must be an int32 device tensor of %d entries' % cin)
  n = rn.lib().ra_conv_wide_packed_floats(cin, co_count)
  if n == 0:
    raise rn.RecAttendError('unsupported wide conv shape Cin=%d Cout=%d (Cin %% 4, <= 1024; Cout 129 .. 512, %% 16)' % (cin, co_count))
  out = torch.empty(n, dtype=torch.float32, device=w.device)
  check(rn.lib().ra_conv_wide_pack_weights_dev(ptr(w), int(cin_w), int(cout), cin, ptr(chan_map), rn.RA_CONV_TRANSPOSED if transposed else 0,
                                               int(co_first), co_count, ptr(out), rn.stream_ptr()), 'ra_conv_wide_pack_weights_dev')
  return out


_WGW_FIELDS = sorted((v, k[len('RA_WGW_PLAN_'):].lower()) for k, v in rn.CONSTANTS.items() if k.startswith('RA_WGW_PLAN_') and k != 'RA_WGW_PLAN_INTS')


def wgrad_wide_plan(cin, cout, B, Hs, Ws, upsample=False):
  """The launch the wide filter gradient takes for x [B,Hs,Ws,cin] and cout output channels (ra_conv3x3_wgrad_wide_plan: host
  only): {'tile_ci', 'tile_co', 'tile_pix', 'taps', 'grid_ci', 'grid_co', 'split', 'tiles_per_part', 'ntiles', 'lds', 'ws_floats'}."""
  rec = (C.c_int * rn.RA_WGW_PLAN_INTS)()
  check(rn.lib().ra_conv3x3_wgrad_wide_plan(int(cin), int(cout), int(B), int(Hs), int(Ws), int(bool(upsample)), rec), 'ra_conv3x3_wgrad_wide_plan')
  return {name: rec[i] for i, name in _WGW_FIELDS}


def wgrad_wide_acc(x, du, gw, gb=None, chan_map=None, transposed=False, upsample=False, ws=None):
  """gw += the filter gradient of the wide 3x3 conv that ran on x [B,Hs,Ws,Cin] and produced du's tensor [B,H,W,Cout], gb += the
  bias gradient (None: not wanted).  gw in the reference layout: [3,3,cin_w,Cout], transposed: [3,3,Cout,cin_w] with flipped
  taps; chan_map (int32 device tensor, or None) sends kernel channel c to filter row chan_map[c], -1 = padding.  ws: a
  workspace to reuse (at least ra_conv3x3_wgrad_wide_workspace_floats floats)."""
  _need_cuda(x, du, gw, gb, ws)
  B, Hs, Ws, cin = x.shape
  H, W, cout = du.shape[1:]
  up = 2 if upsample else 1
  if tuple(du.shape[:3]) != (B, Hs * up, Ws * up):
    raise rn.RecAttendError('wgrad_wide_acc: x of %r and du of %r' % (tuple(x.shape), tuple(du.shape)))
  cin_w = gw.shape[3] if transposed else gw.shape[2]
  if tuple(gw.shape) != ((3, 3, cout, cin_w) if transposed else (3, 3, cin_w, cout)) or (gb is not None and gb.numel() != cout):
    raise rn.RecAttendError('wgrad_wide_acc: gw of %r / gb for %d output channels' % (tuple(gw.shape), cout))
  if chan_map is not None and not (chan_map.is_cuda and chan_map.dtype == torch.int32 and chan_map.numel() == cin):
    raise rn.RecAttendError('wgrad_wide_acc: chan_map must be an int32 device tensor of %d entries' % cin)
  n = rn.lib().ra_conv3x3_wgrad_wide_workspace_floats(cin, cout, B, H, W)
  if n == 0:
    raise rn.RecAttendError('wgrad_wide_acc: unsupported shape Cin=%d Cout=%d (Cin %% 4, <= 1024; Cout 129 .. 512, %% 16)' % (cin, cout))
  if ws is None or ws.numel() < n:
    ws = torch.empty(n, dtype=torch.float32, device=x.device)
  check(rn.lib().ra_conv3x3_wgrad_wide_acc_f32(ptr(x), cin, B, Hs, Ws, int(bool(upsample)), ptr(du), cout, ptr(ws), ws.numel(), ptr(chan_map),
                                               int(cin_w), int(bool(transposed)), ptr(gw), ptr(gb), rn.stream_ptr()),
        'ra_conv3x3_wgrad_wide_acc_f32')
  return gw


# ---- BatchNorm / filter gradient / subsample of the training layers (csrc/ra_bn.hip, ra_bn_wide.hip, ra_wgrad.hip; ra_layer_train).
# wide: the ra_bn_wide_* kernels (C % 4 == 0 up to 512).

_POISON = os.environ.get('RA_POISON')  # a debugging aid: every scratch tensor starts as this value (e.g. "nan") instead of stale memory


def _f(*shape, device):
  if _POISON:
    return torch.full(shape, float(_POISON), dtype=torch.float32, device=device)
  return torch.empty(shape, dtype=torch.float32, device=device)


def bn_workspace(C_, like, ws=None, groups=1, wide=False):
  """ws if it is large enough for `groups` BatchNorm passes over C_ channels, else a new workspace of the library's size."""
  n = groups * (rn.lib().ra_bn_wide_workspace_floats if wide else rn.lib().ra_bn_workspace_floats)(int(C_))
  return ws if ws is not None and ws.numel() >= n else _f(n, device=like.device)


def bn_moments(u, ws=None, out=None, wide=False):
  """(mean, var) [C] of u [..., C] over every other axis, biased (tf.nn.moments, nnlib.py:98); out = (mean, var) to fill."""
  _need_cuda(u, ws)
  C_ = u.shape[-1]
  mean, var = out if out is not None else (_f(C_, device=u.device), _f(C_, device=u.device))
  ws = bn_workspace(C_, u, ws, wide=wide)
  name = 'ra_bn_wide_moments_f32' if wide else 'ra_bn_moments_f32'
  check(getattr(rn.lib(), name)(ptr(u), u.numel() // C_, C_, ptr(ws), ws.numel(), ptr(mean), ptr(var), rn.stream_ptr()), name)
  return mean, var


def conv3x3_train(x, wp, scale, shift, cout, upsample=False, bf16=False, out=None, store_flags=None, moments=True):
  """The training forward's conv3x3 (no ReLU, no pool) -> (u, part, nparts); moments: nparts per-wave channel sums in part, for
  bn_moments_from_partials.  store_flags (bit 0: x is bf16, bit 1: out is bf16): ra_conv3x3_bf16_f32; None: ra_conv3x3_moments_f32."""
  _need_cuda(x, wp, scale, shift, out, f32=False)
  B, Hs, Ws, cin = x.shape
  u = _conv_out(x, cout, 1, upsample, out)
  part = _f(rn.lib().ra_conv3x3_moments_part_floats(int(cout)), device=x.device) if moments else None
  nparts = C.c_int(0)
  head = (ptr(x), cin, None, 0, B, Hs, Ws, int(bool(upsample)), ptr(wp), ptr(scale), ptr(shift), int(cout), 0)
  tail = (ptr(part), part.numel(), C.byref(nparts)) if moments else (None, 0, None)
  if store_flags is None:
    check(rn.lib().ra_conv3x3_moments_f32(*head, int(bool(bf16)), ptr(u), *tail, rn.stream_ptr()), 'ra_conv3x3_moments_f32')
  else:
    check(rn.lib().ra_conv3x3_bf16_f32(*head, 1, ptr(u), *tail, int(store_flags), rn.stream_ptr()), 'ra_conv3x3_bf16_f32')
  return u, part, nparts.value


def bn_moments_from_partials(part, nparts, C_, out=None):
  """(mean, var) [C] from the nparts per-wave channel sums a conv epilogue left (conv3x3_train)."""
  _need_cuda(part)
  mean, var = out if out is not None else (_f(C_, device=part.device), _f(C_, device=part.device))
  check(rn.lib().ra_bn_moments_from_partials_f32(ptr(part), int(nparts), int(C_), ptr(mean), ptr(var), rn.stream_ptr()),
        'ra_bn_moments_from_partials_f32')
  return mean, var


def bn_act_pool(u, mean, var, gamma, beta, relu=True, pool=1, out=None, store_flags=None, wide=False):
  """y = max_pool(relu?(gamma (u - mean) rsqrt(var + 1e-3) + beta)) for u [B,H,W,C]; the four None together: y = pool(relu?(u)).
  store_flags (bit 0: u stored as bf16, bit 1: out, then required, written as bf16): the bf16-storage form (narrow kernels only)."""
  _need_cuda(u, out, f32=False)
  _need_cuda(mean, var, gamma, beta)
  B, H, W, C_ = u.shape
  if out is None:
    out = torch.empty((B, H // pool, W // pool, C_), dtype=torch.float32, device=u.device)
  head = (ptr(u), ptr(mean), ptr(var), ptr(gamma), ptr(beta), C.c_float(BN_EPS), int(relu), int(pool), B, H, W, C_, ptr(out))
  if store_flags is not None:
    assert not wide
    check(rn.lib().ra_bn_act_pool_bf16_f32(*head, int(store_flags), rn.stream_ptr()), 'ra_bn_act_pool_bf16_f32')
  else:
    name = 'ra_bn_wide_act_pool_f32' if wide else 'ra_bn_act_pool_f32'
    check(getattr(rn.lib(), name)(*head, rn.stream_ptr()), name)
  return out


def bn_act_pool_bwd(u, dy, mean, var, gamma, beta, relu=True, pool=1, acc=None, ws=None, du=None, wide=False):
  """The backward of bn_act_pool with the batch statistics differentiated through -> (du, dgamma, dbeta).  acc = (acc_gamma,
  acc_beta), views of a gradient bucket or None: the entry point whose kernel adds dgamma / dbeta there; acc None: the plain one."""
  acc = (None, None) if wide and acc is None else acc  # the wide kernels have the accumulating entry point only
  _need_cuda(u, dy, mean, var, gamma, beta, ws, du, *(acc or ()))
  C_ = u.shape[3]
  du = torch.empty_like(u) if du is None else du
  dgamma, dbeta = _f(C_, device=u.device), _f(C_, device=u.device)
  ws = bn_workspace(C_, u, ws, wide=wide)
  head = (ptr(u), ptr(dy), ptr(mean), ptr(var), ptr(gamma), ptr(beta), C.c_float(BN_EPS), int(relu), int(pool), *u.shape, ptr(ws), ws.numel(),
          ptr(dgamma), ptr(dbeta), ptr(du))
  if acc is None:
    check(rn.lib().ra_bn_act_pool_bwd_f32(*head, rn.stream_ptr()), 'ra_bn_act_pool_bwd_f32')
  else:
    name = 'ra_bn_wide_act_pool_bwd_acc_f32' if wide else 'ra_bn_act_pool_bwd_acc_f32'
    check(getattr(rn.lib(), name)(*head, ptr(acc[0]), ptr(acc[1]), rn.stream_ptr()), name)
  return du, dgamma, dbeta


def bn_wide_moments(u, ws=None):
  """bn_moments on the wide kernels (any C % 4 == 0 up to 512)."""
  return bn_moments(u, ws=ws, wide=True)


def bn_wide_act_pool(u, mean, var, gamma, beta, relu=True, pool=1, out=None):
  """bn_act_pool on the wide kernels, float32 storage."""
  return bn_act_pool(u, mean, var, gamma, beta, relu=relu, pool=pool, out=out, wide=True)


def bn_wide_act_pool_bwd(u, dy, mean, var, gamma, beta, relu=True, pool=1, acc_gamma=None, acc_beta=None, ws=None):
  """bn_act_pool_bwd on the wide kernels; acc_gamma / acc_beta (views of a gradient bucket, or None) receive += in the kernel."""
  return bn_act_pool_bwd(u, dy, mean, var, gamma, beta, relu=relu, pool=pool, acc=(acc_gamma, acc_beta), ws=ws, wide=True)


def bn_act_pool_bwd_reduce(u, dy, mean, var, gamma, beta, relu=True, pool=1, acc=(None, None), ws=None, out=None):
  """First half of the backward on WHOLE-batch statistics: this rank's sums (dgamma, dbeta) into out, also added to acc."""
  _need_cuda(u, dy, mean, var, gamma, beta, ws, *acc)
  C_ = u.shape[3]
  dgamma, dbeta = out if out is not None else (_f(C_, device=u.device), _f(C_, device=u.device))
  ws = bn_workspace(C_, u, ws)
  check(rn.lib().ra_bn_act_pool_bwd_reduce_f32(ptr(u), ptr(dy), ptr(mean), ptr(var), ptr(gamma), ptr(beta), C.c_float(BN_EPS), int(relu), int(pool),
                                               *u.shape, ptr(ws), ws.numel(), ptr(dgamma), ptr(dbeta), ptr(acc[0]), ptr(acc[1]), rn.stream_ptr()),
        'ra_bn_act_pool_bwd_reduce_f32')
  return dgamma, dbeta


def bn_act_pool_bwd_dx(u, dy, mean, var, gamma, beta, dgamma_sum, dbeta_sum, n_total, relu=True, pool=1, du=None):
  """Second half: du from the sums of the whole data-parallel batch of n_total elements per channel."""
  _need_cuda(u, dy, mean, var, gamma, beta, du)
  du = torch.empty_like(u) if du is None else du
  check(rn.lib().ra_bn_act_pool_bwd_dx_f32(ptr(u), ptr(dy), ptr(mean), ptr(var), ptr(gamma), ptr(beta), ptr(dgamma_sum), ptr(dbeta_sum),
                                           C.c_double(n_total), C.c_float(BN_EPS), int(relu), int(pool), *u.shape, ptr(du), rn.stream_ptr()),
        'ra_bn_act_pool_bwd_dx_f32')
  return du


def bn_act_pool_bwd_grouped(U, dY, tabs, G, relu=True, pool=1, store_flags=0, ws=None):
  """The backward of G stacked calls of one layer, U [G * B,H,W,C], in one launch -> (du, dgamma [G,C], dbeta [G,C]).  tabs: device
  table of 6 G pointers {mean, var, gamma, beta, gradient gamma, gradient beta}[G] (the last two receive +=); store_flags as the kernel's."""
  _need_cuda(U, dY, tabs, ws, f32=False)
  N, H, W, C_ = U.shape
  du = torch.empty_like(U)
  dgamma, dbeta = _f(G, C_, device=U.device), _f(G, C_, device=U.device)
  ws = bn_workspace(C_, U, ws, groups=G)
  check(rn.lib().ra_bn_act_pool_bwd_grouped_bf16_f32(ptr(U), ptr(dY), ptr(tabs), int(G), C.c_float(BN_EPS), int(relu), int(pool), N // G, H, W,
                                                     C_, ptr(ws), ws.numel(), ptr(dgamma), ptr(dbeta), ptr(du), int(store_flags),
                                                     rn.stream_ptr()), 'ra_bn_act_pool_bwd_grouped_bf16_f32')
  return du, dgamma, dbeta


def wgrad3x3_workspace_floats(cin, cout, B, H, W):
  return rn.lib().ra_conv3x3_wgrad_workspace_floats(int(cin), int(cout), int(B), int(H), int(W))


def _wgrad3x3_ws(x, du, ws):
  n = wgrad3x3_workspace_floats(x.shape[3], du.shape[3], *du.shape[:3])
  return ws if ws is not None and ws.numel() >= n else _f(n, device=x.device)


def wgrad3x3(x, du, upsample=False, bf16=False, ws=None):
  """(dw [3,3,Cin,Cout], db [Cout]) of the 3x3 conv that ran on x [B,Hs,Ws,Cin] and produced du's tensor [B,H,W,Cout]; upsample: the
  stride-2 transposed form; bf16: bf16 operands, float32 sums."""
  _need_cuda(x, du, ws)
  B, Hs, Ws, cin = x.shape
  cout = du.shape[3]
  dw, db = _f(3, 3, cin, cout, device=x.device), _f(cout, device=x.device)
  ws = _wgrad3x3_ws(x, du, ws)
  name = 'ra_conv3x3_wgrad_bf16ops_f32' if bf16 else 'ra_conv3x3_wgrad_f32'
  check(getattr(rn.lib(), name)(ptr(x), cin, B, Hs, Ws, int(bool(upsample)), ptr(du), cout, ptr(ws), ws.numel(), ptr(dw), ptr(db),
                                rn.stream_ptr()), name)
  return dw, db


def wgrad3x3_acc(x, du, gw, gb=None, chan_map=None, transposed=False, upsample=False, bf16=False, ws=None):
  """gw += wgrad3x3's filter gradient in the reference layout of the filter that ran ([3,3,cin_w,Cout]; transposed: [3,3,Cout,cin_w],
  taps flipped), gb += the bias gradient (None: not wanted).  chan_map (int32 device tensor or None): kernel channel c -> filter row
  chan_map[c], -1 = padding.  x and / or du stored as bf16: the bf16-storage form (bf16 operands)."""
  _need_cuda(x, du, f32=False)
  _need_cuda(gw, gb, ws)
  B, Hs, Ws, cin = x.shape
  ws = _wgrad3x3_ws(x, du, ws)
  head = (ptr(x), cin, B, Hs, Ws, int(bool(upsample)), ptr(du), du.shape[3], ptr(ws), ws.numel(), ptr(chan_map),
          int(gw.shape[3] if transposed else gw.shape[2]), int(bool(transposed)), ptr(gw), ptr(gb))
  fmt = (1 if x.dtype == torch.bfloat16 else 0) | (2 if du.dtype == torch.bfloat16 else 0)
  if fmt:
    check(rn.lib().ra_conv3x3_wgrad_acc_bf16_f32(*head, fmt, rn.stream_ptr()), 'ra_conv3x3_wgrad_acc_bf16_f32')
  else:
    name = 'ra_conv3x3_wgrad_acc_bf16ops_f32' if bf16 else 'ra_conv3x3_wgrad_acc_f32'
    check(getattr(rn.lib(), name)(*head, rn.stream_ptr()), name)
  return gw


def wgrad3x3_multi_acc(tab, n, seg_shape, cout, ws, gw, gb, chan_map=None, cin_w=None, transposed=False, upsample=False, bf16=False):
  """wgrad3x3_acc summed over n calls of one layer in one pass: tab (int64 device tensor, 128 slots) holds the calls' x pointers
  in [0, 64) and du pointers in [64, 128); seg_shape = (B,Hs,Ws,Cin) of every x; ws: wgrad3x3_workspace_floats(Cin, cout, n * B, H, W) floats."""
  _need_cuda(ws, gw, gb)
  B, Hs, Ws, cin = seg_shape
  check(rn.lib().ra_conv3x3_wgrad_multi_acc_f32(tab.data_ptr(), tab.data_ptr() + 8 * 64, int(n), cin, B, Hs, Ws, int(bool(upsample)), int(cout),
                                                ptr(ws), ws.numel(), ptr(chan_map), int(cin_w), int(bool(transposed)), ptr(gw), ptr(gb),
                                                int(bf16), rn.stream_ptr()), 'ra_conv3x3_wgrad_multi_acc_f32')
  return gw


def subsample(x, even=False, out=None):
  """Every second pixel of x [B,2 Hs,2 Ws,C] in both directions -> [B,Hs,Ws,C]: the odd positions (2 i + 1), or the even ones."""
  _need_cuda(x, out)
  B, H, W, C_ = x.shape
  out = _f(B, H // 2, W // 2, C_, device=x.device) if out is None else out
  if tuple(out.shape) != (B, H // 2, W // 2, C_):
    raise rn.RecAttendError('subsample: out of shape %r for x of %r' % (tuple(out.shape), tuple(x.shape)))
  name = 'ra_subsample_even_f32' if even else 'ra_subsample_odd_f32'
  check(getattr(rn.lib(), name)(ptr(x), B, H // 2, W // 2, C_, ptr(out), rn.stream_ptr()), name)
  return out


def fg_head(logits, nsc, no, quantise=False, y_out=None, d_out=None, x=None, packed=None, canvas_plane=None):
  """The head of fg_model: logits [B,H,W,nsc+no] -> (y_out [B,H,W,nsc], d_out [B,H,W,no] or None); quantise: the 8-bit
  round trip floor(v * 255) / 255.  packed [B,H,W,Cp] (with x [B,H,W,D]): the decode engine's packed input image is
  written in the same pass, canvas_plane [B,H,W] zeroed."""
  _need_cuda(logits, y_out, d_out, x, packed, canvas_plane)
  B, H, W, C = logits.shape
  if C != nsc + no:
    raise rn.RecAttendError('fg_head: %d channels for nsc %d + no %d' % (C, nsc, no))
  npix = B * H * W
  f = lambda c: torch.empty((B, H, W, c), dtype=torch.float32, device=logits.device)
  if y_out is None:
    y_out = f(nsc)
  if d_out is None and no:
    d_out = f(no)
  if y_out.numel() != npix * nsc or (no and d_out.numel() != npix * no):
    raise rn.RecAttendError('fg_head: destination sizes')
  D = Cp = 0
  if packed is not None:
    if x is None or x.numel() % npix or packed.numel() % npix:
      raise rn.RecAttendError('fg_head: the packed destination needs x [B,H,W,D]')
    D, Cp = x.numel() // npix, packed.numel() // npix
    if canvas_plane is not None and canvas_plane.numel() != npix:
      raise rn.RecAttendError('fg_head: canvas plane size')
  check(rn.lib().ra_fg_head_f32(ptr(logits), npix, int(nsc), int(no), int(bool(quantise)), ptr(y_out), ptr(d_out if no else None),
                                ptr(x if packed is not None else None), D, ptr(packed), Cp,
                                ptr(canvas_plane if packed is not None else None), rn.stream_ptr()), 'ra_fg_head_f32')
  return y_out, (d_out if no else None)


def conv_wino_supported(cin, cout, pool, H, W):
  return bool(rn.lib().ra_conv_wino_supported(int(cin), int(cout), int(pool), int(H), int(W)))


def pack_wino_weights(w):
  """TF-layout [3,3,Cin,Cout] filter -> transformed filters G g G^T in MFMA B-operand order (numpy, host)."""
  w = _np32(w)
  cin, cout = w.shape[2], w.shape[3]
  n = rn.lib().ra_conv_wino_packed_floats(cin, cout)
  if w.shape[0] != 3 or w.shape[1] != 3 or n == 0:
    raise rn.RecAttendError('unsupported Winograd conv shape %r' % (w.shape,))
  out = np.empty(n, dtype=np.float32)
  check(rn.lib().ra_conv_wino_pack_weights(ptr(w), cin, cout, ptr(out)), 'ra_conv_wino_pack_weights')
  return out


def conv_split_supported(cin, cout, pool, H, W):
  return bool(rn.lib().ra_conv_split_supported(int(cin), int(cout), int(pool), int(H), int(W)))


def pack_split_weights(w, cin_kernel=None, chan_map=None):
  """TF-layout [3,3,Cin,Cout] filter -> its exact three-piece bf16 split in K1s's B-operand order (numpy, host; bf16 pairs in float32 words).
  cin_kernel / chan_map (as pack_conv_weights): the kernel's input has cin_kernel channels, channel c of it is the filter's input
  channel chan_map[c] (-1: a channel the filter does not read — zero rows)."""
  w = _np32(w)
  if cin_kernel is not None or chan_map is not None:
    ck = int(cin_kernel if cin_kernel is not None else len(chan_map))
    cm = list(chan_map) if chan_map is not None else list(range(w.shape[2])) + [-1] * (ck - w.shape[2])
    wk = np.zeros((3, 3, ck, w.shape[3]), np.float32)
    for c, m_ in enumerate(cm[:ck]):
      if m_ >= 0:
        wk[:, :, c, :] = w[:, :, m_, :]
    w = wk
  cin, cout = w.shape[2], w.shape[3]
  n = rn.lib().ra_conv_split_packed_halfs(cin, cout)
  if w.shape[0] != 3 or w.shape[1] != 3 or n == 0:
    raise rn.RecAttendError('unsupported split-precision conv shape %r' % (w.shape,))
  out = np.empty(n, dtype=np.int16)
  check(rn.lib().ra_conv_split_pack_weights(ptr(w), cin, cout, ptr(out)), 'ra_conv_split_pack_weights')
  return out.view(np.float32)  # carried as a float32 tensor like every other packed filter (two bf16 pieces per word)


def pack_split_weights_dev(w, cin, cout, transposed=False):
  """The same packing from a DEVICE filter (the training step: the weights change every step).  cin / cout: the conv's input
  / output channels; transposed: w is laid out [3,3,cout,cin] and the taps flip (a conv2d_transpose filter, or the filter of
  a cnn layer whose data gradient this conv is)."""
  _need_cuda(w)
  n = rn.lib().ra_conv_split_packed_halfs(int(cin), int(cout))
  if n == 0 or w.numel() != 9 * cin * cout:
    raise rn.RecAttendError('unsupported split-precision conv shape Cin=%d Cout=%d' % (cin, cout))
  out = torch.empty(n // 2, dtype=torch.float32, device=w.device)
  check(rn.lib().ra_conv_split_pack_weights_dev(ptr(w.contiguous()), int(cin), int(cout), int(bool(transposed)), ptr(out),
                                                rn.stream_ptr()), 'ra_conv_split_pack_weights_dev')
  return out


def conv_split(x, wp, scale, shift, cout, relu=True, pool=1, out=None, plane=None, plane_chan=-1):
  """conv3x3 SAME + folded BN + ReLU + pool as a direct convolution on the bf16 matrix pipe at float32 accuracy
  (ra_conv_split_f32: three bf16 pieces per operand, six piece products).  x [B,H,W,Cin]; plane [B,H,W]: stands in for channel
  plane_chan of x (ra_conv_split_plane_f32)."""
  _need_cuda(x, wp, scale, shift, out, plane)
  B, H, W, cin = x.shape
  out = _conv_out(x, cout, pool, out=out)
  if plane is not None:
    check(rn.lib().ra_conv_split_plane_f32(ptr(x), B, H, W, cin, ptr(plane), int(plane_chan), ptr(wp), ptr(scale), ptr(shift), int(cout),
                                           int(relu), int(pool), ptr(out), rn.stream_ptr()), 'ra_conv_split_plane_f32')
    return out
  check(rn.lib().ra_conv_split_f32(ptr(x), B, H, W, cin, ptr(wp), ptr(scale), ptr(shift), int(cout), int(relu), int(pool),
                                   ptr(out), rn.stream_ptr()), 'ra_conv_split_f32')
  return out


def conv_wino(x, wp, scale, shift, cout, relu=True, pool=1, out=None):
  """conv3x3 SAME + folded BN + ReLU + pool as Winograd F(2x2,3x3) (ra_conv_wino_f32).  x [B,H,W,Cin]."""
  _need_cuda(x, wp, scale, shift, out)
  B, H, W, cin = x.shape
  out = _conv_out(x, cout, pool, out=out)
  check(rn.lib().ra_conv_wino_f32(ptr(x), B, H, W, cin, ptr(wp), ptr(scale), ptr(shift), int(cout), int(relu), int(pool),
                                  ptr(out), rn.stream_ptr()), 'ra_conv_wino_f32')
  return out


def conv_pair_wino_supported(cin, cout_a, cout_b, pool_b, H, W):
  return bool(rn.lib().ra_conv_pair_wino_supported(int(cin), int(cout_a), int(cout_b), int(pool_b), int(H), int(W)))


def conv_pair_wino(x, wpA, scA, shA, wpB_wino, scB, shB, reluA=True, reluB=True, out=None):
  """The fused pair 8 -> 16 -> 16, pool 2, with layer B as Winograd (ra_conv_pair_wino_f32).  x [B,H,W,8]."""
  _need_cuda(x, wpA, scA, shA, wpB_wino, scB, shB, out)
  B, H, W, _ = x.shape
  out = _conv_out(x, 16, 2, out=out)
  check(rn.lib().ra_conv_pair_wino_f32(ptr(x), B, H, W, ptr(wpA), ptr(scA), ptr(shA), int(reluA), ptr(wpB_wino), ptr(scB),
                                       ptr(shB), int(reluB), ptr(out), rn.stream_ptr()), 'ra_conv_pair_wino_f32')
  return out


def conv_pair16_supported(cin, cout_a, cout_b, pool_b, H, W):
  return bool(rn.lib().ra_conv_pair16_supported(int(cin), int(cout_a), int(cout_b), int(pool_b), int(H), int(W)))


def conv_pair16(x, wpA, scA, shA, wpB, scB, shB, reluA=True, reluB=True, out=None):
  """The fused pair 8 -> 16 -> 16, pool 2, with both layers direct on the bf16 matrix pipe (ra_conv_pair16_f32).  x [B,H,W,8];
  wpA, wpB = pack_conv_weights of the two filters."""
  _need_cuda(x, wpA, scA, shA, wpB, scB, shB, out)
  B, H, W, _ = x.shape
  out = _conv_out(x, 16, 2, out=out)
  check(rn.lib().ra_conv_pair16_f32(ptr(x), B, H, W, ptr(wpA), ptr(scA), ptr(shA), int(reluA), ptr(wpB), ptr(scB), ptr(shB),
                                    int(reluB), ptr(out), rn.stream_ptr()), 'ra_conv_pair16_f32')
  return out


def poison_lds():
  """Test aid: leave NaN in every CU's LDS (see ra_debug_poison_lds)."""
  check(rn.lib().ra_debug_poison_lds(rn.stream_ptr()), 'ra_debug_poison_lds')


def park_xcd(xcd, n_wg, lds_bytes=100 * 1024, millis=100, resident=None, stream=None):
  """Test aid: hold n_wg CUs' worth of LDS on one XCD for `millis` ms (ra_debug_park_xcd); resident: int32 device counter."""
  check(rn.lib().ra_debug_park_xcd(int(xcd), int(n_wg), int(lds_bytes), int(millis), ptr(resident) if resident is not None else None,
                                   rn.stream_ptr() if stream is None else stream.cuda_stream), 'ra_debug_park_xcd')


def conv_pair_supported(cin, cout_a, cout_b):
  return bool(rn.lib().ra_conv_pair_supported(int(cin), int(cout_a), int(cout_b)))


def conv_pair(src, wpA, scA, shA, coutA, wpB, scB, shB, coutB, poolB=1, upsampleA=False,
              reluA=True, reluB=True, out=None, plane=None, plane_chan=-1):
  """Two fused conv layers (A: no pool / optional stride-2 transposed; B: pool 1|2)."""
  _need_cuda(src, wpA, scA, shA, wpB, scB, shB, out)
  B, Hs, Ws, C0 = src.shape
  out = _conv_out(src, coutB, poolB, upsampleA, out)
  check(rn.lib().ra_conv_pair_f32(ptr(src), C0, B, Hs, Ws, int(upsampleA), ptr(wpA), ptr(scA),
                                  ptr(shA), int(coutA), int(reluA), ptr(wpB), ptr(scB), ptr(shB),
                                  int(coutB), int(reluB), int(poolB), ptr(plane), int(plane_chan),
                                  ptr(out), rn.stream_ptr()),
        'ra_conv_pair_f32')
  return out


def first_cache_supported(cin, cout_a, cout_b, pool_b, H, W):
  return bool(rn.lib().ra_conv_first_cache_supported(int(cin), int(cout_a), int(cout_b), int(pool_b), int(H), int(W)))


def first_cache_alloc(B, H, W, device):
  return torch.zeros((rn.lib().ra_conv_first_cache_floats(B, H, W),), dtype=torch.float32, device=device)


def first_cache(img, wpA, cout_a, plane_chan, cache):
  """Once per forward: the image channels' share of the first conv layer (ra_conv_first_cache_f32)."""
  _need_cuda(img, wpA, cache)
  B, H, W, C = img.shape
  assert C == 4
  check(rn.lib().ra_conv_first_cache_f32(ptr(img), B, H, W, ptr(wpA), int(cout_a), int(plane_chan), ptr(cache),
                                         rn.stream_ptr()), 'ra_conv_first_cache_f32')


def fill_rider_ok(t):
  """Can `t` be filled by the rider of conv_pair_fill_cache (contiguous, 16-byte aligned, % 4, < 2 GiB)?"""
  return t.is_contiguous() and t.data_ptr() % 16 == 0 and t.numel() % 4 == 0 and t.numel() * 4 < (1 << 31)


def conv_pair_fill_cache(img, plane, plane_chan, wpA, scA, shA, wpB, scB, shB, coutB, cache, out, reluA=True, reluB=True,
                         fill=None, fill_value=0.0):
  """First timestep (canvas plane all zero): the plain first pair, writing the cache on the way.
  fill: a tensor set to fill_value by the same launch (the decode loop's y_out prefill)."""
  _need_cuda(img, plane, wpA, scA, shA, wpB, scB, shB, cache, out, fill)
  B, H, W = plane.shape
  if fill is not None and not fill_rider_ok(fill):
    raise rn.RecAttendError('conv_pair_fill_cache: the rider fill needs a contiguous, 16-byte aligned tensor of 4k floats < 2 GiB')
  check(rn.lib().ra_conv_pair_fill_cache_rider_f32(ptr(img), ptr(plane), int(plane_chan), B, H, W, ptr(wpA), ptr(scA),
                                                   ptr(shA), int(reluA), ptr(wpB), ptr(scB), ptr(shB), int(coutB),
                                                   int(reluB), ptr(cache), ptr(out), ptr(fill),
                                                   0 if fill is None else fill.numel(), C.c_float(fill_value),
                                                   rn.stream_ptr()),
        'ra_conv_pair_fill_cache_rider_f32')
  return out


def conv_pair_cached(cache, plane, plane_chan, wpA, scA, shA, wpB, scB, shB, coutB, out, reluA=True, reluB=True):
  """Per timestep: the first controller-CNN pair from the cached image part + the canvas plane."""
  _need_cuda(cache, plane, wpA, scA, shA, wpB, scB, shB, out)
  B, H, W = plane.shape
  check(rn.lib().ra_conv_pair_cached_f32(ptr(cache), ptr(plane), int(plane_chan), B, H, W, ptr(wpA), ptr(scA),
                                         ptr(shA), int(reluA), ptr(wpB), ptr(scB), ptr(shB), int(coutB),
                                         int(reluB), ptr(out), rn.stream_ptr()), 'ra_conv_pair_cached_f32')
  return out


def controller(desc, feat, wp, h_last, ctrl_out, gmaps, attn):
  _need_cuda(feat, wp, h_last, ctrl_out, gmaps, attn)
  B = feat.shape[0]
  check(rn.lib().ra_controller_f32(C.byref(desc), ptr(feat), ptr(wp), B, ptr(h_last),
                                   ptr(ctrl_out), ptr(gmaps), ptr(attn), rn.stream_ptr()),
        'ra_controller_f32')


def extract_direct(img, chan0, attn, Fh, Fw, Cp, use_gamma, patch, canvas=None, canvas_chan=-1):
  _need_cuda(img, attn, patch, canvas)
  B, H, W, Ci = img.shape
  check(rn.lib().ra_extract_direct_f32(ptr(img), Ci, chan0, ptr(canvas), int(canvas_chan), ptr(attn),
                                       B, H, W, Fh, Fw, Cp, int(use_gamma), ptr(patch),
                                       rn.stream_ptr()), 'ra_extract_direct_f32')


def extract_conv0_supported(Cp, Fh, Fw, cout, pool):
  return bool(rn.lib().ra_extract_conv0_supported(int(Cp), int(Fh), int(Fw), int(cout), int(pool)))


def extract_conv0(img, chan0, attn, Fh, Fw, use_gamma, patch, w0, scale, shift, cout, relu, y0, canvas=None, canvas_chan=-1):
  """extract_direct + layer 0 of the attention CNN (3x3, BN folded, ReLU, no pool) in one launch (ra_extract_conv0_f32).
  w0 [3,3,4,cout]: the filter in the packed input's channel order; y0 [B,Fh,Fw,cout]."""
  _need_cuda(img, attn, patch, canvas, w0, scale, shift, y0)
  B, H, W, Ci = img.shape
  check(rn.lib().ra_extract_conv0_f32(ptr(img), Ci, chan0, ptr(canvas), int(canvas_chan), ptr(attn), B, H, W, Fh, Fw,
                                      int(use_gamma), ptr(patch), ptr(w0), ptr(scale), ptr(shift), int(cout), int(relu), ptr(y0),
                                      rn.stream_ptr()), 'ra_extract_conv0_f32')


PASTE_Y_PREFILLED, PASTE_CANVAS_FLOORED = rn.RA_PASTE_Y_PREFILLED, rn.RA_PASTE_CANVAS_FLOORED


def paste_direct(patch, pc, attn, beta, disable_overwrite, y_out, y_stride_b, H, W, canvas=None,
                 img=None, canvas_chan=-1, flags=0):
  _need_cuda(patch, attn, canvas, img)
  B, Fh, Fw, Cp = patch.shape
  Ci = 0 if img is None else img.shape[3]
  check(rn.lib().ra_paste_direct_f32(ptr(patch), Cp, pc, ptr(attn), B, H, W, Fh, Fw, C.c_float(beta),
                                     int(disable_overwrite), ptr(canvas), ptr(img), Ci,
                                     int(canvas_chan), ptr(y_out), y_stride_b, int(flags),
                                     rn.stream_ptr()),
        'ra_paste_direct_f32')


def paste_score_direct(patch, pc, attn, beta, disable_overwrite, y_out, y_stride_b, H, W, canvas, flags,
                       h, core, w, bias, s_out_ptr, s_stride_b):
  """paste_direct on a canvas plane + the score MLP of the timestep in the same launch."""
  _need_cuda(patch, attn, canvas, h, core, w, bias)
  B, Fh, Fw, Cp = patch.shape
  K1 = 0 if core is None else core.shape[1]
  check(rn.lib().ra_paste_score_direct_f32(ptr(patch), Cp, pc, ptr(attn), B, H, W, Fh, Fw, C.c_float(beta),
                                           int(disable_overwrite), ptr(canvas), ptr(y_out), y_stride_b,
                                           int(flags), ptr(h), h.shape[1], ptr(core), K1, ptr(w), ptr(bias),
                                           ptr(s_out_ptr), s_stride_b, rn.stream_ptr()),
        'ra_paste_score_direct_f32')


def paste_plan(mode, B, H, W, Fh, Fw, Cp=1, pc=0, has_canvas=True, has_img=False, y_stride_b=None, aligned16=True):
  """ra_paste_plan: which kernel paste_direct / paste_score_direct (mode 'paste') or attn_box_direct (mode 'box') launches on
  these arguments, as a dict kernel ('general' | 'window'), rows, grid_x, threads, lds.  Host only: nothing is launched."""
  rec = (C.c_int * rn.RA_PASTE_PLAN_INTS)()
  stride = H * W if y_stride_b is None else y_stride_b
  check(rn.lib().ra_paste_plan({'paste': 0, 'box': 1}[mode], int(B), int(H), int(W), int(Fh), int(Fw), int(Cp), int(pc),
                               int(bool(has_canvas)), int(bool(has_img)), int(stride), int(bool(aligned16)), rec), 'ra_paste_plan')
  return {'kernel': {rn.RA_PASTE_KERNEL_GENERAL: 'general', rn.RA_PASTE_KERNEL_WINDOW: 'window'}[rec[rn.RA_PASTE_PLAN_KERNEL]],
          'rows': rec[rn.RA_PASTE_PLAN_ROWS], 'grid_x': rec[rn.RA_PASTE_PLAN_GRID_X], 'threads': rec[rn.RA_PASTE_PLAN_THREADS],
          'lds': rec[rn.RA_PASTE_PLAN_LDS]}


RESAMPLE_READ, RESAMPLE_WRITE, RESAMPLE_BOX = rn.RA_RESAMPLE_READ, rn.RA_RESAMPLE_WRITE, rn.RA_RESAMPLE_BOX


def resample_bwd(mode, rec, H, W, Fh, Fw, X=None, chan0=0, C=None, dY=None, Y=None, Q=None, E=None, scale=None, div=None):
  """ra_resample_bwd_f32 (include/recattend.h): the adjoint of one attention resample straight to the gradients of the
  window parameters.  Returns out [B,8] = (d ctr_y, d ctr_x, d size_y, d size_x, d lg_var_y, d lg_var_x, d gamma, 0)."""
  _need_cuda(rec, X, dY, Y, Q, E)  # scale / div: strided [B] views (a column of the record), read with their stride
  B = rec.shape[0]
  if mode == RESAMPLE_READ:
    Cx = X.shape[3]
    C = Cx - chan0 if C is None else C
  else:
    Cx, C = 1, 1
  lib = rn.lib()
  nws = lib.ra_resample_bwd_workspace_floats(B, Fh, C)
  ws = torch.empty(nws, dtype=torch.float32, device=rec.device)
  out = torch.empty((B, 8), dtype=torch.float32, device=rec.device)
  sstride = 0 if scale is None else int(scale.stride(0))
  dstride = 0 if div is None else int(div.stride(0))
  check(lib.ra_resample_bwd_f32(int(mode), ptr(X), int(Cx), int(chan0), int(C), ptr(dY), ptr(Y), ptr(rec), ptr(Q),
                                0 if Q is None else int(Q.shape[3]), ptr(E), 0 if E is None else int(E.shape[3]), B, H, W, Fh, Fw,
                                ptr(scale), sstride, ptr(div), dstride, ptr(ws), nws, ptr(out), rn.stream_ptr()),
        'ra_resample_bwd_f32')
  return out


def attn_box_direct(attn, H, W, Fh, Fw, beta, out, stride_b):
  _need_cuda(attn)
  check(rn.lib().ra_attn_box_direct_f32(ptr(attn), attn.shape[0], H, W, Fh, Fw, C.c_float(beta),
                                        ptr(out), stride_b, rn.stream_ptr()),
        'ra_attn_box_direct_f32')


def dense(x0, W, b, act, out, out_stride_b, x1=None):
  """act: None/'relu'/'sigmoid'/'softmax'/'tanh'.  out may be a view; pass its data ptr."""
  _need_cuda(x0, x1, W, b)
  code = {None: 0, 'relu': 1, 'sigmoid': 2, 'softmax': 3, 'tanh': 4}[act]
  K1 = 0 if x1 is None else x1.shape[1]
  check(rn.lib().ra_dense_f32(ptr(x0), x0.shape[1], ptr(x1), K1, ptr(W), ptr(b), x0.shape[0],
                              W.shape[1], code, ptr(out), out_stride_b, rn.stream_ptr()),
        'ra_dense_f32')


def pack_input(x, d_in, y_in, Cp, packed, canvas_plane=None):
  """canvas_plane: the decode loop's separate canvas [B,H,W], zeroed by the same launch."""
  _need_cuda(x, d_in, y_in, packed, canvas_plane)
  B, H, W, D = x.shape
  Dd = 0 if d_in is None else d_in.shape[3]
  Dy = 0 if y_in is None else y_in.shape[3]
  check(rn.lib().ra_pack_input_plane_f32(ptr(x), D, ptr(d_in), Dd, ptr(y_in), Dy, B, H, W, Cp,
                                         ptr(packed), ptr(canvas_plane), rn.stream_ptr()), 'ra_pack_input_plane_f32')


def canvas_max(img, canvas_chan, ysel, noise):
  _need_cuda(img, ysel, noise)
  B, H, W, Ci = img.shape
  check(rn.lib().ra_canvas_max_f32(ptr(img), Ci, canvas_chan, ptr(ysel), ptr(noise), B, H, W,
                                   rn.stream_ptr()), 'ra_canvas_max_f32')


def gaussian_filter(center, size, lg_var, L, F):
  _need_cuda(center, size, lg_var)
  B = center.shape[0]
  out = torch.empty((B, L, F), dtype=torch.float32, device=center.device)
  check(rn.lib().ra_gaussian_filter_f32(ptr(center), ptr(size), ptr(lg_var), B, L, F, ptr(out),
                                        rn.stream_ptr()), 'ra_gaussian_filter_f32')
  return out


def extract_patch_dense(x, f_y, f_x):
  _need_cuda(x, f_y, f_x)
  B, H, W, D = x.shape
  FH, FW = f_y.shape[2], f_x.shape[2]
  out = torch.empty((B, FH, FW, D), dtype=torch.float32, device=x.device)
  check(rn.lib().ra_extract_patch_dense_f32(ptr(x), ptr(f_y), ptr(f_x), B, H, W, D, FH, FW,
                                            ptr(out), rn.stream_ptr()),
        'ra_extract_patch_dense_f32')
  return out


def affine_act(x, scale, shift, relu=False):
  _need_cuda(x, scale, shift)
  Cc = x.shape[-1]
  out = torch.empty_like(x)
  check(rn.lib().ra_affine_act_f32(ptr(x), ptr(scale), ptr(shift), x.numel() // Cc, Cc,
                                   int(relu), ptr(out), rn.stream_ptr()), 'ra_affine_act_f32')
  return out


def max_pool(x, ratio):
  _need_cuda(x)
  B, H, W, Cc = x.shape
  out = torch.empty((B, -(-H // ratio), -(-W // ratio), Cc), dtype=torch.float32,
                    device=x.device)
  check(rn.lib().ra_max_pool_f32(ptr(x), B, H, W, Cc, int(ratio), ptr(out), rn.stream_ptr()),
        'ra_max_pool_f32')
  return out


def hungarian(weights):
  """Drop-in for hungarian_module.hungarian (modellib.py:406): weights [B,N,M] or [N,M] ->
  (matching, cover_x [...,N,1], cover_y [...,1,M]).  CPU tensors/arrays run the host entry
  point (like the reference's CPU op); CUDA tensors run the device kernel."""
  is_t = isinstance(weights, torch.Tensor)
  two_d = (weights.ndim == 2)
  if weights.ndim not in (2, 3):
    raise rn.RecAttendError('Must have dimension 3 or 2.')  # hungarian.cc:62
  if is_t and weights.is_cuda:
    w = weights.detach().to(torch.float32).contiguous()
    w3 = w[None] if two_d else w
    B, N, M = w3.shape
    m = torch.empty_like(w3)
    cx = torch.empty((B, N), dtype=torch.float32, device=w.device)
    cy = torch.empty((B, M), dtype=torch.float32, device=w.device)
    st = torch.zeros((max(B, 1),), dtype=torch.int32, device=w.device)
    nb = rn.lib().ra_hungarian_dev_workspace_bytes(max(B, 1), N, M)
    ws = torch.empty((nb,), dtype=torch.uint8, device=w.device)
    check(rn.lib().ra_hungarian_f32_dev(ptr(w3), B, N, M, ptr(m), ptr(cx), ptr(cy), ptr(st),
                                        ptr(ws), nb, rn.stream_ptr()), 'ra_hungarian_f32_dev')
    hungarian.last_status = st
    check_match_status(st, 'hungarian')
    cx, cy = cx[:, :, None], cy[:, None, :]
    return (m[0], cx[0], cy[0]) if two_d else (m, cx, cy)
  w = _np32(weights)
  w3 = w[None] if two_d else w
  B, N, M = w3.shape
  m = np.zeros_like(w3)
  cx = np.zeros((B, N), np.float32)
  cy = np.zeros((B, M), np.float32)
  rc = rn.lib().ra_hungarian_f32(ptr(w3), B, N, M, ptr(m), ptr(cx), ptr(cy))
  if rc < 0:
    check(rc, 'ra_hungarian_f32')
  hungarian.last_status = rc
  cx, cy = cx[:, :, None], cy[:, None, :]
  if two_d:
    m, cx, cy = m[0], cx[0], cy[0]
  if is_t:
    return torch.from_numpy(m), torch.from_numpy(cx), torch.from_numpy(cy)
  return m, cx, cy


hungarian.last_status = 0


def check_match_status(status, what='Hungarian'):
  """Per-example status of the device solver (int32 [B], include/recattend.h): a negative code is
  where the reference LOG(FATAL)s (hungarian.cc:124-127,146-160,184-188,446-450) — raise instead of
  carrying a partial matching into the loss; 1 is the outer 1000-iteration cap, where the
  reference logs an error and returns the partial matching (hungarian.cc:363-377) — warn."""
  if status is None or isinstance(status, int):
    worst, capped = (status or 0), (status == 1)
  else:
    worst = int(status.min().item())
    capped = bool((status == 1).any().item())
  if worst < 0:
    raise rn.RecAttendError('%s: the matching solver stopped with code %d (an iteration cap the '
                            'reference aborts on, hungarian.cc LOG(FATAL))' % (what, worst))
  if capped:
    import warnings
    warnings.warn('%s: outer iteration cap reached, partial matching returned (hungarian.cc:363-377)'
                  % what)


# --------------------------------------------------------------------------------------
# loss / statistics head (csrc/ra_loss.hip)
# --------------------------------------------------------------------------------------
STAT_NAMES = ('loss', 'box_loss', 'segm_loss', 'conf_loss', 'iou_soft', 'iou_soft_box',
              'wt_cov_soft', 'unwt_cov_soft', 'iou_hard', 'wt_cov_hard', 'unwt_cov_hard', 'dice',
              'count_acc', 'dic', 'dic_abs')  # RA_STAT_* order


def pair_stats(a, b, want=('iou_soft', 'iou_hard', 'dice_hard', 'sum_a', 'sum_b'), a_tmajor=False):
  """One pass over a [B,N,H,W] and b [B,M,H,W]: pairwise soft IoU, IoU / DICE of (a > 0.5), and
  the per-instance sums (modellib.f_iou / f_dice pairwise=True, full_model.py:981,1064-1073).
  a_tmajor: a is stored [N,B,H,W] (the training step's timestep-major masks), read in place through strides."""
  a, b = a.contiguous(), b.contiguous()
  _need_cuda(a, b)
  if a_tmajor:
    N, B, H, W = a.shape
  else:
    B, N, H, W = a.shape
  M = b.shape[1]
  dev = a.device
  n = rn.lib().ra_pair_stats_workspace_floats(B, H * W)
  ws = torch.empty((n,), dtype=torch.float32, device=dev)
  out = {}
  for k, shp in (('iou_soft', (B, N, M)), ('iou_hard', (B, N, M)), ('dice_hard', (B, N, M)),
                 ('sum_a', (B, N)), ('sum_b', (B, M)), ('inter', (B, N, M)), ('sum_a_hard', (B, N))):
    out[k] = torch.empty(shp, dtype=torch.float32, device=dev) if k in want else None
  if a_tmajor:
    check(rn.lib().ra_pair_stats_strided_f32(ptr(a), H * W, B * H * W, ptr(b), B, N, M, H * W, ptr(ws), n, ptr(out['iou_soft']),
                                             ptr(out['iou_hard']), ptr(out['dice_hard']), ptr(out['sum_a']), ptr(out['sum_b']),
                                             ptr(out['inter']), ptr(out['sum_a_hard']), rn.stream_ptr()), 'ra_pair_stats_strided_f32')
    return out
  check(rn.lib().ra_pair_stats_f32(ptr(a), ptr(b), B, N, M, H * W, ptr(ws), n, ptr(out['iou_soft']),
                                   ptr(out['iou_hard']), ptr(out['dice_hard']), ptr(out['sum_a']),
                                   ptr(out['sum_b']), ptr(out['inter']), ptr(out['sum_a_hard']),
                                   rn.stream_ptr()), 'ra_pair_stats_f32')
  return out


def gt_box(y_gt, padding_ratio, min_padding, want_box=True, want_ws=False):
  """modellib.get_gt_box (modellib.py:663-701), center_shift_ratio = 0: params [B,T,8], box (want_ws: also the
  workspace holding the min / max / sum partials, which knob_setup reads)."""
  y_gt = y_gt.contiguous()
  _need_cuda(y_gt)
  B, T, H, W = y_gt.shape
  params = torch.empty((B, T, 8), dtype=torch.float32, device=y_gt.device)
  box = torch.empty((B, T, H, W), dtype=torch.float32, device=y_gt.device) if want_box else None
  n = rn.lib().ra_gt_box_workspace_floats(B, T)
  ws = torch.empty((n,), dtype=torch.float32, device=y_gt.device)
  check(rn.lib().ra_gt_box_f32(ptr(y_gt), B, T, H, W, C.c_float(padding_ratio),
                               C.c_float(min_padding), ptr(ws), n, ptr(params), ptr(box),
                               rn.stream_ptr()), 'ra_gt_box_f32')
  return (params, box, ws) if want_ws else (params, box)


def knob_setup(gt_ws, B, T, pad, shift, u_box, u_segm, sched, min_padding, timescale):
  """The step's noisy ground-truth attention (ctr, size [B,T,2]) and knob masks [B,T,1] from gt_box's partials: one launch
  (full_model.py:567-577,596-625)."""
  pad, shift, u_box, u_segm, sched = (t.contiguous() for t in (pad, shift, u_box, u_segm, sched))
  _need_cuda(gt_ws, pad, shift, u_box, u_segm, sched)
  dev = gt_ws.device
  ctr, size = torch.empty((B, T, 2), dtype=torch.float32, device=dev), torch.empty((B, T, 2), dtype=torch.float32, device=dev)
  kb, ks = torch.empty((B, T, 1), dtype=torch.float32, device=dev), torch.empty((B, T, 1), dtype=torch.float32, device=dev)
  check(rn.lib().ra_knob_setup_f32(ptr(gt_ws), B, T, ptr(pad), ptr(shift), ptr(u_box), ptr(u_segm), ptr(sched), C.c_float(min_padding),
                                   int(bool(timescale)), ptr(ctr), ptr(size), ptr(kb), ptr(ks), rn.stream_ptr()), 'ra_knob_setup_f32')
  return ctr, size, kb, ks


def box_iou_rects(box, params):
  """f_iou (soft) of box [B,H,W] against the T rectangles of gt_box's params [B,T,8] -> [B,T]."""
  box, params = box.contiguous(), params.contiguous()
  _need_cuda(box, params)
  B, H, W = box.shape
  T = params.shape[1]
  out = torch.empty((B, T), dtype=torch.float32, device=box.device)
  ws = torch.empty((rn.lib().ra_box_iou_rects_workspace_floats(B),), dtype=torch.float32, device=box.device)
  check(rn.lib().ra_box_iou_rects_f32(ptr(box), ptr(params), B, T, H, W, ptr(ws), ws.numel(), ptr(out), rn.stream_ptr()),
        'ra_box_iou_rects_f32')
  return out


def segm_match(iou, s_gt):
  """modellib.f_segm_match (modellib.py:382-415) on device; returns (match [B,N,N], status [B])."""
  iou, s_gt = iou.contiguous(), s_gt.contiguous()
  _need_cuda(iou, s_gt)
  B, N, _ = iou.shape
  nb = rn.lib().ra_segm_match_workspace_bytes(B, N)
  ws = torch.empty((nb,), dtype=torch.uint8, device=iou.device)
  match = torch.empty_like(iou)
  status = torch.zeros((B,), dtype=torch.int32, device=iou.device)
  check(rn.lib().ra_segm_match_f32(ptr(iou), ptr(s_gt), B, N, ptr(ws), nb, ptr(match), ptr(status),
                                   rn.stream_ptr()), 'ra_segm_match_f32')
  return match, status


def segm_match_host(iou, s_gt, block=None, threads=16):
  """modellib.f_segm_match with the Hungarian problems solved on HOST cores, side by side, as a host function of the current stream
  (a host node under graph capture): ra_segm_match_host_f32.  block: (pinned uint8 host tensor, device float scratch) kept by the
  caller for as long as a captured graph may replay the call (None: a fresh one is made and returned).  -> (match, status, block)."""
  iou, s_gt = iou.contiguous(), s_gt.contiguous()
  _need_cuda(iou, s_gt)
  B, N, _ = iou.shape
  nb = rn.lib().ra_segm_match_host_block_bytes(B, N)
  if block is None or block[0].numel() < nb or block[1].numel() < B * N * N:
    block = (torch.empty((nb,), dtype=torch.uint8).pin_memory(), torch.empty((B * N * N,), dtype=torch.float32, device=iou.device))
  match = torch.empty_like(iou)
  status = torch.zeros((B,), dtype=torch.int32, device=iou.device)
  check(rn.lib().ra_segm_match_host_f32(ptr(iou), ptr(s_gt), B, N, ptr(block[1]), block[0].data_ptr(), block[0].numel(), int(threads),
                                        ptr(match), ptr(status), rn.stream_ptr()), 'ra_segm_match_host_f32')
  return match, status, block


def loss_stats(iou_soft, iou_hard, dice, match_real, iou_box, match_box, s_out, s_gt, sum_gt,
               fixed_order=False, segm_loss_fn='iou', loss_mix_ratio=1.0):
  """Every scalar of full_model.py:941-1081 -> float32 [len(STAT_NAMES)] on the device."""
  ts = [t.contiguous() for t in (iou_soft, iou_hard, dice, match_real, iou_box, match_box, s_out,
                                 s_gt, sum_gt)]
  _need_cuda(*ts)
  B, T = s_gt.shape
  out = torch.empty((len(STAT_NAMES),), dtype=torch.float32, device=s_gt.device)
  fn = {'iou': 0, 'wt_cov': 1}[segm_loss_fn]
  n = rn.lib().ra_loss_stats_workspace_floats(B)
  ws = torch.empty((n,), dtype=torch.float32, device=s_gt.device)
  check(rn.lib().ra_loss_stats_f32(*[ptr(t) for t in ts], B, T, int(bool(fixed_order)), fn,
                                   C.c_float(loss_mix_ratio), ptr(ws), n, ptr(out), rn.stream_ptr()),
        'ra_loss_stats_f32')
  return out


# --------------------------------------------------------------------------------------
# evaluation post-processing and metrics (csrc/ra_eval.hip)
# --------------------------------------------------------------------------------------
EVAL_NAMES = ('sbd', 'wt_cov', 'unwt_cov', 'fg_iou', 'fg_dice', 'avg_fp', 'avg_fn', 'count_acc',
              'count_mse', 'dic', 'dic_abs', 'num_obj', 'count_out')  # RA_EVAL_* order
EVALI_NAMES = ('obj_pr', 'obj_re', 'pix_pr', 'pix_re', 'has_out', 'is_gt')  # RA_EVALI_* order


def postprocess(y_out, s_out, thresh, fg=None, want_union=False):
  """apply_confidence -> apply_one_label -> apply_threshold [-> mask_foreground] in one pass
  (utils/postprocess.py:5-52,139-147): (y_bin [B,T,H,W], s_hard [B,T], union [B,H,W] | None)."""
  y_out, s_out = y_out.contiguous(), s_out.contiguous()
  fg = None if fg is None else fg.contiguous()
  _need_cuda(y_out, s_out, fg)
  B, T, H, W = y_out.shape
  y_bin = torch.empty_like(y_out)
  s_hard = torch.empty((B, T), dtype=torch.float32, device=y_out.device)
  uni = torch.empty((B, H, W), dtype=torch.float32, device=y_out.device) if want_union else None
  check(rn.lib().ra_postprocess_f32(ptr(y_out), ptr(s_out), B, T, H, W, C.c_float(thresh),
                                    ptr(fg), ptr(y_bin),
                                    ptr(s_hard), ptr(uni), rn.stream_ptr()), 'ra_postprocess_f32')
  return y_bin, s_hard, uni


def union_over_instances(y):
  """y [B,T,H,W] -> max over T [B,H,W] (analysis.py:547,570)."""
  y = y.contiguous()
  _need_cuda(y)
  B, T, H, W = y.shape
  out = torch.empty((B, H, W), dtype=torch.float32, device=y.device)
  check(rn.lib().ra_union_f32(ptr(y), B, T, H * W, ptr(out), rn.stream_ptr()), 'ra_union_f32')
  return out


def dilate(y, radius=2):
  """cv2.dilate(plane, ones((2 radius + 1,) * 2)) on every [H,W] plane of y [..., H, W] (postprocess.py:63-72)."""
  y = y.contiguous()
  _need_cuda(y)
  H, W = y.shape[-2:]
  out = torch.empty_like(y)
  check(rn.lib().ra_dilate_f32(ptr(y), y.numel() // (H * W), H, W, int(radius), ptr(out), rn.stream_ptr()), 'ra_dilate_f32')
  return out


def resize_linear(y, H, W):
  """cv2.resize(plane, (W, H), interpolation=INTER_LINEAR) on every plane of y [..., Hs, Ws] (postprocess.py:103-104)."""
  y = y.contiguous()
  _need_cuda(y)
  Hs, Ws = y.shape[-2:]
  out = torch.empty(y.shape[:-2] + (int(H), int(W)), dtype=torch.float32, device=y.device)
  check(rn.lib().ra_resize_linear_f32(ptr(y), y.numel() // (Hs * Ws), Hs, Ws, int(H), int(W), ptr(out), rn.stream_ptr()),
        'ra_resize_linear_f32')
  return out


def bilateral5(y, sigma_color=10.0, sigma_space=10.0):
  """cv2.bilateralFilter(plane, 5, sigma_color, sigma_space) on every plane of y [..., H, W] (postprocess.py:105)."""
  y = y.contiguous()
  _need_cuda(y)
  H, W = y.shape[-2:]
  out = torch.empty_like(y)
  check(rn.lib().ra_bilateral5_f32(ptr(y), y.numel() // (H * W), H, W, C.c_float(sigma_color), C.c_float(sigma_space), ptr(out),
                                   rn.stream_ptr()), 'ra_bilateral5_f32')
  return out


def remove_tiny(y_bin, sizes, conf, threshold):
  """In place: instance planes of at most `threshold` pixels are zeroed, their conf too."""
  _need_cuda(y_bin, sizes, conf)
  B, T, H, W = y_bin.shape
  check(rn.lib().ra_remove_tiny_f32(ptr(y_bin), ptr(sizes.contiguous()), ptr(conf), B, T, H * W,
                                    C.c_float(threshold), rn.stream_ptr()), 'ra_remove_tiny_f32')


def eval_metrics(y_bin, y_gt, s_gt, fg_a=None, fg_b=None):
  """Every per-image statistic of analysis.py:314-760 for binary outputs y_bin and ground truth
  y_gt [B,T,H,W]: dict(iou_pairwise [B,T,T], stats [B,len(EVAL_NAMES)], inst [B,len(EVALI_NAMES),T])."""
  y_bin, y_gt, s_gt = y_bin.contiguous(), y_gt.contiguous(), s_gt.contiguous()
  _need_cuda(y_bin, y_gt, s_gt)
  B, T, H, W = y_bin.shape
  dev = y_bin.device
  if fg_a is None:
    fg_a = union_over_instances(y_bin)
  if fg_b is None:
    fg_b = union_over_instances(y_gt)
  main = pair_stats(y_bin, y_gt, want=('inter', 'sum_a', 'sum_b'))
  ua, ub = fg_a.view(B, 1, H, W), fg_b.view(B, 1, H, W)
  fg = pair_stats(ua, ub, want=('inter', 'sum_a', 'sum_b'))
  a_fgb = pair_stats(y_bin, ub, want=('inter',))['inter'].view(B, T).contiguous()
  b_fga = pair_stats(ua, y_gt, want=('inter',))['inter'].view(B, T).contiguous()
  iou = torch.empty((B, T, T), dtype=torch.float32, device=dev)
  stats = torch.empty((B, len(EVAL_NAMES)), dtype=torch.float32, device=dev)
  inst = torch.empty((B, len(EVALI_NAMES), T), dtype=torch.float32, device=dev)
  check(rn.lib().ra_eval_metrics_f32(ptr(main['inter']), ptr(main['sum_a']), ptr(main['sum_b']),
                                     ptr(s_gt.contiguous()), ptr(fg['inter']), ptr(fg['sum_a']),
                                     ptr(fg['sum_b']), ptr(a_fgb), ptr(b_fga), B, T, ptr(iou), ptr(stats),
                                     ptr(inst), rn.stream_ptr()), 'ra_eval_metrics_f32')
  return {'iou_pairwise': iou, 'stats': stats, 'inst': inst, 'sizes': main['sum_a']}


def random_transform(x, padding, off_y, off_x, flip_v=False, flip_h=False, transpose=False, out=None):
  """image_ops.random_transformation for given draws on x [N,H,W,C] (or [N,H,W] planes); out: a contiguous tensor of x's
  shape to write into (not x itself)."""
  x = x.contiguous()
  _need_cuda(x, out)
  shape = x.shape
  N, H, W = shape[0], shape[1], shape[2]
  Cc = shape[3] if x.dim() == 4 else 1
  if out is None or tuple(out.shape) != tuple(shape) or not out.is_contiguous() or out.dtype != x.dtype or out.data_ptr() == x.data_ptr():
    out = torch.empty_like(x)
  check(rn.lib().ra_random_transform_f32(ptr(x), N, H, W, Cc, int(padding), int(off_y), int(off_x),
                                         int(bool(flip_v)), int(bool(flip_h)), int(bool(transpose)),
                                         ptr(out), rn.stream_ptr()), 'ra_random_transform_f32')
  return out


def colour_jitter(x, hue_delta, saturation_factor, brightness_delta, contrast_factor):
  """image_ops.py:99-103 for given draws on x [B,H,W,3] (ra_colour_jitter_f32)."""
  x = x.contiguous()
  _need_cuda(x)
  B, H, W, Cc = x.shape
  if Cc != 3:
    raise rn.RecAttendError('colour jitter needs an RGB image (last dimension 3)')
  out = torch.empty_like(x)
  n = rn.lib().ra_colour_jitter_workspace_floats(B)
  ws = torch.empty((n,), dtype=torch.float32, device=x.device)
  check(rn.lib().ra_colour_jitter_f32(ptr(x), B, H * W, C.c_float(hue_delta), C.c_float(saturation_factor), C.c_float(brightness_delta),
                                      C.c_float(contrast_factor), ptr(ws), n, ptr(out), rn.stream_ptr()), 'ra_colour_jitter_f32')
  return out


def fill(t, value):
  """t[...] = value as a library launch (keeps framework kernels out of the captured forward)."""
  _need_cuda(t)
  check(rn.lib().ra_fill_f32(ptr(t), t.numel(), C.c_float(value), rn.stream_ptr()), 'ra_fill_f32')
  return t


def tickets_alloc(slots, device):
  """Scratch for `slots` ticketed launches (ra_tile_tickets_bind, include/recattend.h): zeroed by tickets_bind."""
  n = slots * rn.lib().ra_tile_tickets_slot_bytes() // 4
  return torch.zeros((n,), dtype=torch.float32, device=device)


def tickets_bind(t):
  """Zero the scratch on the current stream and make it current for this thread's persistent conv launches: their
  workgroups draw tiles from per-XCD pools instead of walking a fixed list (robust against company on the GPU).
  Returns True if bound; tickets_unbind() ends it.  The launches must all go to the current stream."""
  _need_cuda(t)
  fill(t, 0.0)
  rc = rn.lib().ra_tile_tickets_bind(ptr(t), t.numel() * 4 // rn.lib().ra_tile_tickets_slot_bytes())
  if rc < 0:
    check(rc, 'ra_tile_tickets_bind')
  return rc == 1


def tickets_unbind():
  rn.lib().ra_tile_tickets_bind(None, 0)


def greedy_match(score, out=None):
  """modellib.f_greedy_match with matched == 0 (modellib.py:365-379): score [B,T] -> [B,T]."""
  score = score.contiguous()
  _need_cuda(score, out)
  if out is None:
    out = torch.empty_like(score)
  check(rn.lib().ra_greedy_match_f32(ptr(score), score.shape[0], score.shape[1], ptr(out),
                                     rn.stream_ptr()), 'ra_greedy_match_f32')
  return out


def weighted_sum(w, y, out):
  """out[b] = sum_t w[b,t] * y[b,t] for y [B,T,H,W] (box_model.py:487-499)."""
  w = w.contiguous()
  _need_cuda(w, y, out)
  B, T, H, W = y.shape
  check(rn.lib().ra_weighted_sum_f32(ptr(w), ptr(y), B, T, H * W, ptr(out), rn.stream_ptr()),
        'ra_weighted_sum_f32')


# ---------------------------------------------------------------------------- Cityscapes output stage


def sem_foreground(sem, H, W, thresh=0.3):
  """cityscapes_eval.py:166-176: the foreground mask [B,H,W] of a semantic map sem [B,Hs,Ws,C] (channel-last) at the labels'
  size — one channel: resized > thresh; several: resized channel 0 (background) <= 1 - thresh (ra_sem_foreground_f32)."""
  sem = sem.contiguous()
  _need_cuda(sem)
  B, Hs, Ws, Cc = sem.shape
  fg = torch.empty((B, int(H), int(W)), dtype=torch.float32, device=sem.device)
  check(rn.lib().ra_sem_foreground_f32(ptr(sem), B, Hs, Ws, Cc, int(H), int(W), C.c_float(thresh), ptr(fg), rn.stream_ptr()),
        'ra_sem_foreground_f32')
  return fg


def instance_class_vote(y, sem, conf=None):
  """analysis.py:235-261 for y [B,T,H,W] and the semantic map sem [B,Hs,Ws,C] at network size: vote [B,T,C] = the mean over
  the image of y * resized(sem); with conf [B,T] also (class_idx, label_id) int32 [B,T] from the same finishing launch
  (ra_instance_class_vote_f32).  Returns vote, or (vote, class_idx, label_id)."""
  y, sem = y.contiguous(), sem.contiguous()
  conf = None if conf is None else conf.contiguous()
  _need_cuda(y, sem, conf)
  B, T, H, W = y.shape
  Bs, Hs, Ws, Cc = sem.shape
  if Bs != B or (conf is not None and tuple(conf.shape) != (B, T)):
    raise rn.RecAttendError('instance_class_vote: y %s, sem %s, conf %s do not belong together' % (
        tuple(y.shape), tuple(sem.shape), None if conf is None else tuple(conf.shape)))
  dev = y.device
  n = rn.lib().ra_instance_class_vote_workspace_floats(B, T, H, W, Cc)
  ws = torch.empty((max(n, 1),), dtype=torch.float32, device=dev)
  vote = torch.empty((B, T, Cc), dtype=torch.float32, device=dev)
  idx = torch.empty((B, T), dtype=torch.int32, device=dev) if conf is not None else None
  lab = torch.empty((B, T), dtype=torch.int32, device=dev) if conf is not None else None
  check(rn.lib().ra_instance_class_vote_f32(ptr(y), ptr(sem), B, T, H, W, Hs, Ws, Cc, ptr(conf), ptr(ws), n, ptr(vote), ptr(idx),
                                            ptr(lab), rn.stream_ptr()), 'ra_instance_class_vote_f32')
  return vote if conf is None else (vote, idx, lab)


def instance_class_pick(vote, conf):
  """analysis.py:232,251-261 on vote [B,T,C], conf [B,T]: (class_idx, label_id) int32 [B,T]; -1 = not written."""
  vote, conf = vote.contiguous(), conf.contiguous()
  _need_cuda(vote, conf)
  B, T, Cc = vote.shape
  idx = torch.empty((B, T), dtype=torch.int32, device=vote.device)
  lab = torch.empty((B, T), dtype=torch.int32, device=vote.device)
  check(rn.lib().ra_instance_class_pick_f32(ptr(vote), ptr(conf), B, T, Cc, ptr(idx), ptr(lab), rn.stream_ptr()),
        'ra_instance_class_pick_f32')
  return idx, lab


# ---------------------------------------------------------------------------- ... behind a label-image segmentation
LABEL_VOTE_MAX_T = 32   # instances per launch of ra_label_vote_sweep_f32 / ra_label_planes_f32
LABEL_VOTE_MAX_K = 16   # thresholds per sweep
# label value of class 1 .. 8 (person .. bicycle, analysis.py:203-210) under each convention of a label image
LABEL_CLASS_IDS = {
    'labelIds': (24, 25, 26, 27, 28, 31, 32, 33),  # *_labelIds.png (helpers/labels.py: id)
    'trainIds': (11, 12, 13, 14, 15, 16, 17, 18),  # *_labelTrainIds.png (helpers/labels.py: trainId)
    'lrr': (12, 13, 14, 15, 16, 17, 18, 19),       # cityscapes_eval.py:213-216
}


def label_class_lut(ids='labelIds'):
  """np.uint8[256]: label value -> 0 (background or ignored) or 1 .. 8 = person .. bicycle, for ids in LABEL_CLASS_IDS."""
  if ids not in LABEL_CLASS_IDS:
    raise rn.RecAttendError('label_class_lut: ids must be one of %s, got %r' % (', '.join(sorted(LABEL_CLASS_IDS)), ids))
  lut = np.zeros(256, np.uint8)
  for c, v in enumerate(LABEL_CLASS_IDS[ids]):
    lut[v] = c + 1
  return lut


def _label_vote_args(who, y, labels, lut):
  """The checks ra_label_vote_sweep_f32 and ra_label_planes_f32 share; -> (B, T, H, W, lut as contiguous uint8[256])."""
  for name, t, dt, nd in (('y', y, torch.float32, 4), ('labels', labels, torch.uint8, 3)):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
      raise rn.RecAttendError('%s: %s must be a CUDA (HIP) tensor; there is no CPU fallback' % (who, name))
    if t.dtype != dt or t.dim() != nd:
      raise rn.RecAttendError('%s: %s must be a %s tensor of %d dimensions, got %s %s' % (who, name, dt, nd, t.dtype, tuple(t.shape)))
    if not t.is_contiguous():
      raise rn.RecAttendError('%s: %s must be contiguous, got strides %s for shape %s' % (who, name, tuple(t.stride()), tuple(t.shape)))
  B, T, H, W = y.shape
  if tuple(labels.shape) != (B, H, W):
    raise rn.RecAttendError('%s: labels %s do not belong to y %s (expected %s)' % (who, tuple(labels.shape), tuple(y.shape), (B, H, W)))
  if T < 1 or T > LABEL_VOTE_MAX_T:
    raise rn.RecAttendError('%s: y has T = %d instances (1 <= T <= %d)' % (who, T, LABEL_VOTE_MAX_T))
  lut = np.ascontiguousarray(lut.detach().cpu().numpy() if isinstance(lut, torch.Tensor) else lut)
  if lut.dtype != np.uint8 or lut.shape != (256,):
    raise rn.RecAttendError('%s: lut must be uint8[256], got %s %s' % (who, lut.dtype, lut.shape))
  if lut.max() > 8:
    raise rn.RecAttendError('%s: lut[%d] = %d: a lut entry is 0 or a class 1 .. 8' % (who, int(lut.argmax()), int(lut.max())))
  return B, T, H, W, lut


def label_vote_sweep(y, labels, lut, thresholds, conf, remove_tiny=400):
  """cityscapes_eval.py:183-189 + analysis.py:232-261 behind a label-image segmentation, every threshold from one read of y
  (ra_label_vote_sweep_f32): y float32 [B,T,H,W] (after upsample and apply_confidence), labels uint8 [B,H,W], lut uint8[256]
  on the host (label_class_lut), thresholds a sequence of K <= 16 floats in any order, conf float32 [B,T], remove_tiny a
  non-negative integer.  Returns a dict of device tensors with a leading K axis: counts int32 [K,B,T,8], sizes int32 [K,B,T],
  conf float32, keep uint8, vote float32 [K,B,T,9], class_idx, label_id int32 (-1 = not written)."""
  who = 'label_vote_sweep'
  B, T, H, W, lut = _label_vote_args(who, y, labels, lut)
  th = np.ascontiguousarray(np.asarray(thresholds, np.float64).reshape(-1))
  K = int(th.size)
  if K < 1 or K > LABEL_VOTE_MAX_K:
    raise rn.RecAttendError('%s: thresholds has K = %d entries (1 <= K <= %d)' % (who, K, LABEL_VOTE_MAX_K))
  if np.isnan(th).any():
    raise rn.RecAttendError('%s: thresholds holds a NaN' % who)
  if not isinstance(conf, torch.Tensor) or not conf.is_cuda:
    raise rn.RecAttendError('%s: conf must be a CUDA (HIP) tensor; there is no CPU fallback' % who)
  if conf.dtype != torch.float32 or tuple(conf.shape) != (B, T):
    raise rn.RecAttendError('%s: conf must be float32 %s, got %s %s' % (who, (B, T), conf.dtype, tuple(conf.shape)))
  if int(remove_tiny) != remove_tiny or remove_tiny < 0:
    raise rn.RecAttendError('%s: remove_tiny must be a non-negative integer (a pixel count), got %r' % (who, remove_tiny))
  conf = conf.contiguous()
  dev = y.device
  new = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
  out = {'counts': new((K, B, T, 8), torch.int32), 'sizes': new((K, B, T), torch.int32), 'keep': new((K, B, T), torch.uint8),
         'conf': new((K, B, T), torch.float32), 'vote': new((K, B, T, 9), torch.float32),
         'class_idx': new((K, B, T), torch.int32), 'label_id': new((K, B, T), torch.int32)}
  check(rn.lib().ra_label_vote_sweep_f32(ptr(y), ptr(labels), ptr(lut), B, T, H, W, ptr(th), K, ptr(conf), int(remove_tiny),
                                         ptr(out['counts']), ptr(out['sizes']), ptr(out['keep']), ptr(out['conf']),
                                         ptr(out['vote']), ptr(out['class_idx']), ptr(out['label_id']), rn.stream_ptr()),
        'ra_label_vote_sweep_f32')
  return out


def label_planes(y, labels, lut, thresh, keep=None):
  """One threshold's binary planes [B,T,H,W] from y and a label image in one read and one write (ra_label_planes_f32):
  apply_one_label -> apply_threshold(thresh) -> mask_foreground(lut[labels] > 0) -> remove_tiny as keep uint8 [B,T] (None:
  keep all), bit-equal to those ops for thresh >= 0."""
  who = 'label_planes'
  B, T, H, W, lut = _label_vote_args(who, y, labels, lut)
  if keep is not None:
    if not isinstance(keep, torch.Tensor) or not keep.is_cuda:
      raise rn.RecAttendError('%s: keep must be a CUDA (HIP) tensor; there is no CPU fallback' % who)
    if keep.dtype != torch.uint8 or tuple(keep.shape) != (B, T):
      raise rn.RecAttendError('%s: keep must be uint8 %s, got %s %s' % (who, (B, T), keep.dtype, tuple(keep.shape)))
    keep = keep.contiguous()
  if np.isnan(float(thresh)):
    raise rn.RecAttendError('%s: thresh is a NaN' % who)
  y_bin = torch.empty_like(y)
  check(rn.lib().ra_label_planes_f32(ptr(y), ptr(labels), ptr(lut), B, T, H, W, C.c_double(float(thresh)), ptr(keep), ptr(y_bin),
                                     rn.stream_ptr()), 'ra_label_planes_f32')
  return y_bin


# ---------------------------------------------------------------------------- Cityscapes instance-level AP: the matching step
MAX_GT = rn.RA_OVERLAP_MAX_GT  # distinct ids per image: a constant of the kernels, resting on no measurement of the dataset
OVERLAP_MAX_T = 32   # predictions per launch of ra_instance_overlap_f32
OVERLAP_MAX_B = 65535  # images per launch (the grid's y extent)


def _need_cuda_i32(t, what):
  if not t.is_cuda:
    raise rn.RecAttendError('recattend kernels need CUDA (HIP) tensors; got a CPU tensor for %s. There is no CPU fallback.' % what)
  if t.dtype != torch.int32:
    raise rn.RecAttendError('%s must be an int32 tensor, got %s' % (what, t.dtype))
  if not t.is_contiguous():
    raise rn.RecAttendError('%s must be contiguous, got strides %s for shape %s' % (what, tuple(t.stride()), tuple(t.shape)))


def gt_instance_catalog(gt_ids, check_status=True, names=None):
  """instances2dict.py:37-40 on the device: gt_ids int32 [B,H,W] (the values of *_gtFine_instanceIds.png) -> (ids, pixels,
  count): int32 [B,MAX_GT] the distinct ids of every image in ascending order (-1 beyond count) and their pixel counts, int32
  [B] how many there are (ra_gt_instance_catalog_i32).  check_status (one device-to-host copy of B ints): an image with an
  id outside [0, 65535] or with more than MAX_GT distinct ids raises RecAttendError naming it (names[b], else its index);
  with check_status=False the status words are returned as a fourth tensor instead."""
  _need_cuda_i32(gt_ids, 'gt_ids')
  if gt_ids.dim() != 3 or min(gt_ids.shape) < 1:
    raise rn.RecAttendError('gt_instance_catalog: gt_ids must be [B,H,W], got %s' % (tuple(gt_ids.shape),))
  B, H, W = gt_ids.shape
  if H * W >= 1 << 31 or B > OVERLAP_MAX_B:
    raise rn.RecAttendError('gt_instance_catalog: B=%d, H * W = %d (B <= %d, H * W < 2^31)' % (B, H * W, OVERLAP_MAX_B))
  dev = gt_ids.device
  n = rn.lib().ra_gt_instance_catalog_workspace_ints(B, H, W)
  ws = torch.empty((max(n, 1),), dtype=torch.int32, device=dev)
  ids = torch.empty((B, MAX_GT), dtype=torch.int32, device=dev)
  pixels = torch.empty((B, MAX_GT), dtype=torch.int32, device=dev)
  count = torch.empty((B,), dtype=torch.int32, device=dev)
  status = torch.empty((B,), dtype=torch.int32, device=dev)
  check(rn.lib().ra_gt_instance_catalog_i32(ptr(gt_ids), B, H, W, ptr(ws), n, ptr(ids), ptr(pixels), ptr(count), ptr(status),
                                            rn.stream_ptr()), 'ra_gt_instance_catalog_i32')
  if not check_status:
    return ids, pixels, count, status
  _raise_gt_status(status, names, 'gt_instance_catalog')
  return ids, pixels, count


def _raise_gt_status(status, names, who):
  """The catalogue's status words [B] (one device-to-host copy): the first image with one set raises, named."""
  for b, st in enumerate(status.cpu().tolist()):
    if st:
      why = []
      if st & rn.RA_GT_STATUS_RANGE:
        why.append('an instance id outside [0, 65535]')
      if st & rn.RA_GT_STATUS_COUNT:
        why.append('more than %d distinct instance ids' % MAX_GT)
      raise rn.RecAttendError('%s: image %s has %s' % (who, names[b] if names is not None else b, ' and '.join(why)))


def instance_overlap(y, gt_ids, catalog):
  """evalInstanceLevelSemanticLabeling.py:306-307,:333 for every prediction and ground-truth entry at once: y float32
  [B,T,H,W] (a pixel belongs to prediction t where y != 0), gt_ids int32 [B,H,W], catalog = gt_instance_catalog(gt_ids) ->
  (inter int32 [B,T,MAX_GT], pred_pixels int32 [B,T]) (ra_instance_overlap_f32).  Exact integer counts."""
  _need_cuda(y)
  _need_cuda_i32(gt_ids, 'gt_ids')
  ids, count = catalog[0], catalog[2]
  _need_cuda_i32(ids, 'catalog ids')
  _need_cuda_i32(count, 'catalog count')
  if y.dim() != 4 or gt_ids.dim() != 3 or min(y.shape) < 1:
    raise rn.RecAttendError('instance_overlap: y must be [B,T,H,W] and gt_ids [B,H,W], got %s and %s' % (
        tuple(y.shape), tuple(gt_ids.shape)))
  B, T, H, W = y.shape
  if tuple(gt_ids.shape) != (B, H, W) or tuple(ids.shape) != (B, MAX_GT) or tuple(count.shape) != (B,):
    raise rn.RecAttendError('instance_overlap: y %s, gt_ids %s, catalog ids %s, count %s do not belong together' % (
        tuple(y.shape), tuple(gt_ids.shape), tuple(ids.shape), tuple(count.shape)))
  if T > OVERLAP_MAX_T or H * W >= 1 << 31 or B > OVERLAP_MAX_B:
    raise rn.RecAttendError('instance_overlap: B=%d, T=%d, H * W = %d (B <= %d, T <= %d, H * W < 2^31)' % (
        B, T, H * W, OVERLAP_MAX_B, OVERLAP_MAX_T))
  dev = y.device
  n = rn.lib().ra_instance_overlap_workspace_ints(B, T, H, W)
  ws = torch.empty((max(n, 1),), dtype=torch.int32, device=dev)
  inter = torch.empty((B, T, MAX_GT), dtype=torch.int32, device=dev)
  pred = torch.empty((B, T), dtype=torch.int32, device=dev)
  check(rn.lib().ra_instance_overlap_f32(ptr(y), ptr(gt_ids), ptr(ids), ptr(count), B, T, H, W, ptr(ws), n, ptr(inter), ptr(pred),
                                         rn.stream_ptr()), 'ra_instance_overlap_f32')
  return inter, pred


# ---------------------------------------------------------------------------- Cityscapes pixel-level evaluation
PIXEL_LABELS = rn.RA_PIXEL_LABELS  # label ids 0 .. 33
PIXEL_TILE = rn.RA_PIXEL_TILE      # pixels per tile of the confusion kernel; one workgroup per tile up to 2048 / B tiles per image
SEM_MIN_C, SEM_MAX_C = 2, 9        # channels of a semantic map the arg-max takes: background + up to the eight thing labels


def _need_dev(t, dtype, what):
  if not isinstance(t, torch.Tensor) or not t.is_cuda:
    raise rn.RecAttendError('recattend kernels need CUDA (HIP) tensors; got a CPU tensor for %s. There is no CPU fallback.' % what)
  if t.dtype != dtype:
    raise rn.RecAttendError('%s must be a %s tensor, got %s' % (what, str(dtype).replace('torch.', ''), t.dtype))
  if not t.is_contiguous():
    raise rn.RecAttendError('%s must be contiguous, got strides %s for shape %s' % (what, tuple(t.stride()), tuple(t.shape)))


def _check_sem(who, sem, size):
  _need_dev(sem, torch.float32, 'sem')
  if size is None or len(size) != 2:
    raise rn.RecAttendError('%s: a semantic map needs size=(H, W), got %r' % (who, size))
  H, W = int(size[0]), int(size[1])
  if sem.dim() != 4 or min(sem.shape) < 1 or not SEM_MIN_C <= sem.shape[3] <= SEM_MAX_C:
    raise rn.RecAttendError('%s: sem must be [B,Hs,Ws,C] with %d <= C <= %d, got %s' % (who, SEM_MIN_C, SEM_MAX_C, tuple(sem.shape)))
  B, Hs, Ws, _ = sem.shape
  if H < 1 or W < 1 or H * W >= 1 << 31 or Hs * Ws >= 1 << 31 or B > OVERLAP_MAX_B:
    raise rn.RecAttendError('%s: B=%d, %d x %d -> %d x %d (B <= %d, planes of 1 .. 2^31 - 1 pixels)' % (who, B, Hs, Ws, H, W, OVERLAP_MAX_B))
  return H, W


def sem_labels(sem, size):
  """The label image of the pre-stage's semantic map (ra_sem_labels_u8): sem float32 [B,Hs,Ws,C] (channel 0 the background,
  2 <= C <= 9), size = (H, W) -> uint8 [B,H,W].  Every channel is resized with the linear resample of sem_foreground /
  instance_class_vote, the first maximum wins, channel 0 -> label 0, channel c >= 1 -> the id of CITYSCAPES_LABELS[c - 1]."""
  H, W = _check_sem('sem_labels', sem, size)
  B, Hs, Ws, Cc = sem.shape
  labels = torch.empty((B, H, W), dtype=torch.uint8, device=sem.device)
  check(rn.lib().ra_sem_labels_u8(ptr(sem), B, Hs, Ws, Cc, H, W, ptr(labels), rn.stream_ptr()), 'ra_sem_labels_u8')
  return labels


def pixel_confusion(pred, gt_ids, gt_labels=None, catalog=None, size=None, conf=None, names=None, check_status=True):
  """evaluatePair of evalPixelLevelSemanticLabeling.py (:532-615) for B images (ra_pixel_confusion_u8 / _sem_f32).  pred: a
  uint8 label tensor [B,H,W], or a float32 semantic map [B,Hs,Ws,C] together with size = (H, W) — then the prediction is
  what sem_labels(pred, size) gives, evaluated inside the kernel.  gt_ids int32 [B,H,W]: *_gtFine_instanceIds.png values;
  gt_labels uint8 [B,H,W]: *_gtFine_labelIds.png values, or None: id < 1000 ? id : id // 1000.  catalog: what
  gt_instance_catalog(gt_ids) returned, built here when None.  conf: an int64 [34,34] device tensor that is ADDED to (a
  fresh zero one when None).  Returns {'conf': that tensor, 'inst_tp', 'inst_cat_tp': int32 [B,MAX_GT] per catalogue slot,
  'catalog'}.  An image with a ground-truth or predicted label above 33 raises RecAttendError naming it (names[b], else its
  index), from one device-to-host copy of B status words; with check_status=False the words come back as 'status'
  instead, and the pixels with such a label are in no cell of conf."""
  who = 'pixel_confusion'
  fused = isinstance(pred, torch.Tensor) and pred.dtype == torch.float32
  if fused:
    H, W = _check_sem(who, pred, size)
  else:
    _need_dev(pred, torch.uint8, 'pred (a uint8 label image, or a float32 semantic map with size=)')
    if pred.dim() != 3 or min(pred.shape) < 1:
      raise rn.RecAttendError('%s: pred must be [B,H,W], got %s' % (who, tuple(pred.shape)))
    H, W = pred.shape[1:]
    if size is not None and (int(size[0]), int(size[1])) != (H, W):
      raise rn.RecAttendError('%s: size %r does not match the label image %s' % (who, tuple(size), tuple(pred.shape)))
  B = pred.shape[0]
  _need_cuda_i32(gt_ids, 'gt_ids')
  if gt_labels is not None:
    _need_dev(gt_labels, torch.uint8, 'gt_labels')
  if tuple(gt_ids.shape) != (B, H, W) or (gt_labels is not None and tuple(gt_labels.shape) != (B, H, W)):
    raise rn.RecAttendError('%s: pred %s (size %d x %d), gt_ids %s, gt_labels %s do not belong together' % (
        who, tuple(pred.shape), H, W, tuple(gt_ids.shape), None if gt_labels is None else tuple(gt_labels.shape)))
  if H * W >= 1 << 31 or B > OVERLAP_MAX_B:
    raise rn.RecAttendError('%s: B=%d, H * W = %d (B <= %d, H * W < 2^31)' % (who, B, H * W, OVERLAP_MAX_B))
  if conf is not None:
    _need_dev(conf, torch.int64, 'conf')
    if tuple(conf.shape) != (PIXEL_LABELS, PIXEL_LABELS):
      raise rn.RecAttendError('%s: conf must be [%d,%d], got %s' % (who, PIXEL_LABELS, PIXEL_LABELS, tuple(conf.shape)))
  if names is not None and len(names) != B:
    raise rn.RecAttendError('%s: %d names for %d images' % (who, len(names), B))
  if catalog is not None:
    ids, count = catalog[0], catalog[2]
    _need_cuda_i32(ids, 'catalog ids')
    _need_cuda_i32(count, 'catalog count')
    if tuple(ids.shape) != (B, MAX_GT) or tuple(count.shape) != (B,):
      raise rn.RecAttendError('%s: gt_ids %s, catalog ids %s, count %s do not belong together' % (
          who, tuple(gt_ids.shape), tuple(ids.shape), tuple(count.shape)))
  else:
    catalog = gt_instance_catalog(gt_ids, names=names)
    ids, count = catalog[0], catalog[2]
  dev = gt_ids.device
  if conf is None:
    conf = torch.zeros((PIXEL_LABELS, PIXEL_LABELS), dtype=torch.int64, device=dev)
  n = rn.lib().ra_pixel_confusion_workspace_ints(B, H, W)
  ws = torch.empty((max(n, 1),), dtype=torch.int32, device=dev)
  inst_tp = torch.empty((B, MAX_GT), dtype=torch.int32, device=dev)
  inst_cat_tp = torch.empty((B, MAX_GT), dtype=torch.int32, device=dev)
  status = torch.empty((B,), dtype=torch.int32, device=dev)
  tail = (ptr(gt_ids), ptr(gt_labels), ptr(ids), ptr(count), B, H, W, ptr(ws), n, ptr(conf), ptr(inst_tp), ptr(inst_cat_tp),
          ptr(status), rn.stream_ptr())
  if fused:
    _, Hs, Ws, Cc = pred.shape
    check(rn.lib().ra_pixel_confusion_sem_f32(ptr(pred), Hs, Ws, Cc, *tail), 'ra_pixel_confusion_sem_f32')
  else:
    check(rn.lib().ra_pixel_confusion_u8(ptr(pred), *tail), 'ra_pixel_confusion_u8')
  out = {'conf': conf, 'inst_tp': inst_tp, 'inst_cat_tp': inst_cat_tp, 'catalog': catalog}
  if not check_status:
    out['status'] = status
    return out
  _raise_pixel_status(status, names, who)
  return out


def _raise_pixel_status(status, names, who):
  """The confusion kernel's status words [B] (a tensor: one device-to-host copy; or host values): the first image with one
  set raises, named."""
  for b, st in enumerate(status.cpu().tolist() if isinstance(status, torch.Tensor) else [int(v) for v in status]):
    if st:
      why = []
      if st & rn.RA_PIXEL_STATUS_GT:
        why.append('a ground-truth label above %d' % (PIXEL_LABELS - 1))
      if st & rn.RA_PIXEL_STATUS_PRED:
        why.append('a predicted label above %d' % (PIXEL_LABELS - 1))
      raise rn.RecAttendError('%s: image %s has %s' % (who, names[b] if names is not None else b, ' and '.join(why)))


# ---------------------------------------------------------------------------- evaluating the pre-stage fg_model
FG_STAT_NAMES = ('inter_soft', 'sum_soft', 'sum_gt', 'inter_hard', 'sum_hard', 'seg_ce', 'ori_ce', 'ori_correct', 'mask')  # RA_FG_STAT_*
FG_SWEEP_MAX_K = rn.RA_FG_SWEEP_MAX_K


def fg_statistics(logits, y_gt, d_gt, nsc, no):
  """The sums behind the statistics of fg_model.py:196-248, in one pass over the logits [..., nsc + no] of the pre-stage
  (ra_fg_stats_f32): y_gt [..., nsc] (or [...] for nsc == 1), d_gt [..., 8] or None -> {name: float} over FG_STAT_NAMES,
  float64.  The hard quantities are taken on the logits ([logit > 0]; [logit == max logit], every maximum; the first maximum
  of the orientation logits), not on the rounded probabilities: the two agree in exact arithmetic, and float32 rounding of a
  softmax must not invent ties.  One device-to-host copy of nine doubles."""
  return dict(zip(FG_STAT_NAMES, fg_stat_sums(logits, y_gt, d_gt, nsc, no).cpu().tolist()))


def fg_stat_sums(logits, y_gt, d_gt, nsc, no):
  """fg_statistics without the copy to the host: the RA_FG_STAT_COUNT sums as a float64 device tensor, in the order of
  FG_STAT_NAMES (what ra_fg_loss_bwd_f32 reads)."""
  nsc, no = int(nsc), int(no)
  if not 1 <= nsc <= 16 or no not in (0, 8):
    raise rn.RecAttendError('fg_statistics: nsc %d (1 .. 16), no %d (0 | 8)' % (nsc, no))
  if (d_gt is not None) != bool(no):
    raise rn.RecAttendError('fg_statistics: d_gt goes with no = 8 and only with it (no = %d, d_gt %s)' % (
        no, 'given' if d_gt is not None else 'missing'))
  _need_cuda(logits, y_gt, d_gt)
  if logits.dim() < 1 or logits.shape[-1] != nsc + no or logits.numel() == 0:
    raise rn.RecAttendError('fg_statistics: logits %s for nsc %d + no %d channels' % (tuple(logits.shape), nsc, no))
  npix = logits.numel() // (nsc + no)
  if y_gt.numel() != npix * nsc or (no and d_gt.numel() != npix * no):
    raise rn.RecAttendError('fg_statistics: logits %s, y_gt %s, d_gt %s do not belong together' % (
        tuple(logits.shape), tuple(y_gt.shape), None if d_gt is None else tuple(d_gt.shape)))
  dev = logits.device
  n = rn.lib().ra_fg_stats_workspace_bytes(npix)
  ws = torch.empty((max(n // 8, 1),), dtype=torch.float64, device=dev)
  sums = torch.empty((len(FG_STAT_NAMES),), dtype=torch.float64, device=dev)
  check(rn.lib().ra_fg_stats_f32(ptr(logits), ptr(y_gt), ptr(d_gt), npix, nsc, no, ptr(ws), n, ptr(sums), rn.stream_ptr()),
        'ra_fg_stats_f32')
  return sums


FG_SEGM_LOSS_FN = {'iou': 0, 'bce': 1}  # segm_loss_fn of ra_fg_loss_bwd_f32 (fg_model.py:228-231)


def fg_loss_backward(logits, y_gt, d_gt, nsc, no, segm_loss_fn, sums, upstream=1.0, status=None):
  """dL/dlogits of the loss head of fg_model.py:196-248 (ra_fg_loss_bwd_f32): logits [..., nsc + no], y_gt [..., nsc] (or
  [...] for nsc == 1), d_gt [..., 8] or None, segm_loss_fn 'iou' | 'bce', sums: the float64 device tensor fg_stat_sums gave for
  the same tensors (read on the device).  Returns (dlogits, status): status is an int32 device tensor of one word, 1 when the
  batch has orientation classes and no foreground pixel (the orientation gradient is then 0 and the guarded optimizer
  entries skip the step), else 0; pass `status` to have it written in place."""
  nsc, no = int(nsc), int(no)
  if segm_loss_fn not in FG_SEGM_LOSS_FN:
    raise rn.RecAttendError('fg_loss_backward: segm_loss_fn %r (iou | bce)' % (segm_loss_fn,))
  if not 1 <= nsc <= 16 or no not in (0, 8):
    raise rn.RecAttendError('fg_loss_backward: nsc %d (1 .. 16), no %d (0 | 8)' % (nsc, no))
  if (d_gt is not None) != bool(no):
    raise rn.RecAttendError('fg_loss_backward: d_gt goes with no = 8 and only with it (no = %d, d_gt %s)' % (
        no, 'given' if d_gt is not None else 'missing'))
  _need_cuda(logits, y_gt, d_gt)
  if not sums.is_cuda:
    raise rn.RecAttendError('fg_loss_backward: sums must stay on the device (fg_stat_sums); there is no CPU path')
  if logits.dim() < 1 or logits.shape[-1] != nsc + no or logits.numel() == 0:
    raise rn.RecAttendError('fg_loss_backward: logits %s for nsc %d + no %d channels' % (tuple(logits.shape), nsc, no))
  npix = logits.numel() // (nsc + no)
  if y_gt.numel() != npix * nsc or (no and d_gt.numel() != npix * no):
    raise rn.RecAttendError('fg_loss_backward: logits %s, y_gt %s, d_gt %s do not belong together' % (
        tuple(logits.shape), tuple(y_gt.shape), None if d_gt is None else tuple(d_gt.shape)))
  if sums.dtype != torch.float64 or sums.numel() != len(FG_STAT_NAMES) or not sums.is_contiguous():
    raise rn.RecAttendError('fg_loss_backward: sums must be the %d float64 values of fg_stat_sums' % len(FG_STAT_NAMES))
  if status is None:
    status = torch.empty((1,), dtype=torch.int32, device=logits.device)
  elif status.dtype != torch.int32 or status.numel() < 1 or not status.is_cuda:
    raise rn.RecAttendError('fg_loss_backward: status must be an int32 device tensor')
  dlogits = torch.empty_like(logits)
  check(rn.lib().ra_fg_loss_bwd_f32(ptr(logits), ptr(y_gt), ptr(d_gt), npix, nsc, no, FG_SEGM_LOSS_FN[segm_loss_fn], ptr(sums),
                                    C.c_float(float(upstream)), ptr(dlogits), ptr(status), rn.stream_ptr()), 'ra_fg_loss_bwd_f32')
  return dlogits, status


def _sweep_thresholds(thresholds):
  thr = np.ascontiguousarray(np.asarray(thresholds, dtype=np.float32).reshape(-1))
  if not 1 <= thr.size <= FG_SWEEP_MAX_K:
    raise rn.RecAttendError('fg_sweep_counts: %d thresholds (1 .. %d)' % (thr.size, FG_SWEEP_MAX_K))
  return thr


def fg_sweep_counts_device(src, gt, thresholds, out=None):
  """ra_fg_sweep_counts_f32 without the copy to the host: src float32 [N,Hs,Ws], gt uint8 [N,H,W], thresholds (host values)
  -> int64 device tensor [N, RA_FG_SWEEP_SLOTS] (count_a at [:, :K], sum_ab at [:, 16:16 + K], sum_b at [:, 32])."""
  thr = _sweep_thresholds(thresholds)
  if not (isinstance(src, torch.Tensor) and isinstance(gt, torch.Tensor)) or not src.is_cuda or not gt.is_cuda:
    raise rn.RecAttendError('fg_sweep_counts needs CUDA (HIP) tensors; got a CPU tensor. There is no CPU fallback.')
  if src.dtype != torch.float32 or gt.dtype != torch.uint8 or not src.is_contiguous() or not gt.is_contiguous():
    raise rn.RecAttendError('fg_sweep_counts: src must be contiguous float32 and gt contiguous uint8, got %s and %s' % (src.dtype, gt.dtype))
  if src.dim() != 3 or gt.dim() != 3 or src.shape[0] != gt.shape[0] or min(src.shape) < 1 or min(gt.shape) < 1:
    raise rn.RecAttendError('fg_sweep_counts: src must be [N,Hs,Ws] and gt [N,H,W], got %s and %s' % (tuple(src.shape), tuple(gt.shape)))
  N, Hs, Ws = src.shape
  H, W = gt.shape[1:]
  if H * W >= 1 << 31 or Hs * Ws >= 1 << 31 or N > 65535:
    raise rn.RecAttendError('fg_sweep_counts: N=%d, %d x %d -> %d x %d (N <= 65535, planes below 2^31 pixels)' % (N, Hs, Ws, H, W))
  if out is None:
    out = torch.empty((N, rn.RA_FG_SWEEP_SLOTS), dtype=torch.int64, device=src.device)
  elif tuple(out.shape) != (N, rn.RA_FG_SWEEP_SLOTS) or out.dtype != torch.int64 or not out.is_cuda or not out.is_contiguous():
    raise rn.RecAttendError('fg_sweep_counts: out must be a contiguous int64 device tensor [%d, %d]' % (N, rn.RA_FG_SWEEP_SLOTS))
  check(rn.lib().ra_fg_sweep_counts_f32(ptr(src), ptr(gt), N, Hs, Ws, H, W, ptr(thr), int(thr.size), ptr(out), rn.stream_ptr()),
        'ra_fg_sweep_counts_f32')
  return out


def fg_sweep_counts(src, gt, thresholds):
  """fg_model_eval.py:134-178 up to the analyzers' sums, for every threshold at once: src float32 [N,Hs,Ws] (the soft
  foreground at network size), gt uint8 [N,H,W] (the full-size labels summed over the instances; 2 and more where instances
  overlap) -> {'count_a' [N,K], 'sum_ab' [N,K], 'sum_b' [N], 'pixels': H * W, 'thresholds'}: NumPy int64 on the host,
  with a = [bilateralFilter(resize(src), 5, 10, 10) > threshold], which is never written (ra_fg_sweep_counts_f32)."""
  c = fg_sweep_counts_device(src, gt, thresholds).cpu().numpy()
  K = len(_sweep_thresholds(thresholds))
  return {'count_a': c[:, :K].copy(), 'sum_ab': c[:, FG_SWEEP_MAX_K:FG_SWEEP_MAX_K + K].copy(), 'sum_b': c[:, 2 * FG_SWEEP_MAX_K].copy(),
          'pixels': int(gt.shape[1] * gt.shape[2]), 'thresholds': [float(t) for t in _sweep_thresholds(thresholds)]}


# ---------------------------------------------------- the decode loop's evaluator from instance-id images (csrc/ra_instance_eval.hip)
INS_EVAL_MAX_K = rn.RA_INS_EVAL_MAX_K
INS_EVAL_MAX_PIXELS = 1 << 24  # every count stays exact in the float32 ra_eval_metrics_f32 takes


def _ins_eval_thresholds(thresholds):
  thr = np.ascontiguousarray(np.asarray(thresholds, dtype=np.float32).reshape(-1))
  if not 1 <= thr.size <= INS_EVAL_MAX_K:
    raise rn.RecAttendError('instance_eval_counts: %d thresholds (1 .. %d)' % (thr.size, INS_EVAL_MAX_K))
  if not (thr >= 0).all():
    raise rn.RecAttendError('instance_eval_counts: thresholds %s; every one must be >= 0 (below zero the zeros of the planes that '
                            'lost the arg-max pass apply_threshold, which this pass does not count)' % thr.tolist())
  return thr


def ins_eval_threshold_pos(thresholds):
  """pos int32 [K] on the host: pos[k] = how many of the thresholds lie strictly below thresholds[k] (float32 compares,
  ra_instance_eval_threshold_pos: the order the counting pass itself uses).  A pixel whose winner-map word holds n passes
  threshold k as given iff n > pos[k]."""
  thr = _ins_eval_thresholds(thresholds)
  pos = np.zeros((thr.size,), dtype=np.int32)
  check(rn.lib().ra_instance_eval_threshold_pos(ptr(thr), int(thr.size), ptr(pos)), 'ra_instance_eval_threshold_pos')
  return pos


def _ins_eval_map(who, map_out, shape, device):
  """The winner map's tensor: map_out as it is after a check, or a new uint16 tensor of `shape`."""
  if map_out is None:
    return torch.empty(shape, dtype=torch.uint16, device=device)
  if not isinstance(map_out, torch.Tensor) or not map_out.is_cuda:
    raise rn.RecAttendError('%s needs CUDA (HIP) tensors; got a CPU tensor. There is no CPU fallback.' % who)
  if map_out.dtype != torch.uint16 or tuple(map_out.shape) != tuple(shape) or not map_out.is_contiguous():
    raise rn.RecAttendError('%s: map_out must be contiguous uint16 %s, got %s %s' % (who, tuple(shape), map_out.dtype, tuple(map_out.shape)))
  return map_out


def instance_eval_counts(yc, gt_ids, inst_id, thresholds, fg=None, morph=False, check_fg=True, want_map=False, map_out=None):
  """ra_instance_eval_counts_f32: the chain of full_model_eval.py:112-124 behind apply_confidence — upsample [-> morph] ->
  apply_one_label -> per threshold apply_threshold [-> mask_foreground] — as exact counts, for all thresholds in one pass.
  yc float32 [B,T,Hs,Ws] (y_out * s_out at network size), gt_ids int32 [B,Hf,Wf], inst_id int32 [B,T] (the id of ground-truth
  slot j, -1 = empty: assemble_labels(..., want=('inst_id',)) at NETWORK size), thresholds: 1 .. 16 host values >= 0 in any
  order, fg uint8 [B,Hf,Wf] 0 / 1 or None, morph: dilate 5 x 5 behind the filter -> (inter int32 [B,K,T,T + 1], area_b int32
  [B,T]) on the device: inter[b,k,t,j] = the pixels of prediction t on ground-truth slot j at threshold k (column T: on no
  listed instance; a prediction's area is its row sum), area_b[b,j] = the pixels of slot j.  check_fg: look at fg's largest
  value (one device-to-host copy) and refuse anything but 0 / 1, which is where the chain's mask_foreground is a mask.
  want_map: also return the winner map, uint16 [B,Hf,Wf] (ra_instance_eval_counts_map_f32; into map_out when given) — the word
  of a pixel is n << 8 | t*, t* the prediction that holds it and n the number of thresholds, in ascending order, it passes (0:
  none, and then the whole word is 0); paint_instances turns it into pictures.  inter and area_b are the same bits either way."""
  thr = _ins_eval_thresholds(thresholds)
  ts = (yc, gt_ids, inst_id) + (() if fg is None else (fg,))
  if not all(isinstance(t, torch.Tensor) for t in ts) or not all(t.is_cuda for t in ts):
    raise rn.RecAttendError('instance_eval_counts needs CUDA (HIP) tensors; got a CPU tensor. There is no CPU fallback.')
  if yc.dtype != torch.float32 or gt_ids.dtype != torch.int32 or inst_id.dtype != torch.int32 or not all(t.is_contiguous() for t in ts):
    raise rn.RecAttendError('instance_eval_counts: yc must be contiguous float32, gt_ids and inst_id contiguous int32, got %s, %s, %s' % (
        yc.dtype, gt_ids.dtype, inst_id.dtype))
  if yc.dim() != 4 or gt_ids.dim() != 3 or min(yc.shape) < 1 or min(gt_ids.shape) < 1 or gt_ids.shape[0] != yc.shape[0] or \
      tuple(inst_id.shape) != tuple(yc.shape[:2]):
    raise rn.RecAttendError('instance_eval_counts: yc must be [B,T,Hs,Ws], gt_ids [B,Hf,Wf] and inst_id [B,T], got %s, %s, %s' % (
        tuple(yc.shape), tuple(gt_ids.shape), tuple(inst_id.shape)))
  B, T, Hs, Ws = yc.shape
  Hf, Wf = gt_ids.shape[1:]
  if not (T <= LABELS_MAX_T and Hf * Wf <= INS_EVAL_MAX_PIXELS and Hs * Ws < 1 << 31 and B <= 65535):
    raise rn.RecAttendError('instance_eval_counts: T=%d, B=%d, %d x %d -> %d x %d (T <= %d, B <= 65535, Hf * Wf <= 2^24 so that '
                            'every count is exact in float32, Hs * Ws < 2^31)' % (T, B, Hs, Ws, Hf, Wf, LABELS_MAX_T))
  if fg is not None:
    if fg.dtype != torch.uint8 or tuple(fg.shape) != tuple(gt_ids.shape):
      raise rn.RecAttendError('instance_eval_counts: fg must be uint8 %s, got %s %s' % (tuple(gt_ids.shape), fg.dtype, tuple(fg.shape)))
    if check_fg and int(fg.max()) > 1:
      raise rn.RecAttendError('instance_eval_counts: fg holds %d; a foreground mask is 0 / 1' % int(fg.max()))
  K = int(thr.size)
  inter = torch.empty((B, K, T, T + 1), dtype=torch.int32, device=yc.device)
  area_b = torch.empty((B, T), dtype=torch.int32, device=yc.device)
  if want_map or map_out is not None:
    wmap = _ins_eval_map('instance_eval_counts', map_out, (B, Hf, Wf), yc.device)
    check(rn.lib().ra_instance_eval_counts_map_f32(ptr(yc), ptr(gt_ids), ptr(inst_id), ptr(fg), B, T, Hs, Ws, Hf, Wf,
                                                   int(bool(morph)), ptr(thr), K, ptr(inter), ptr(area_b), ptr(wmap),
                                                   rn.stream_ptr()), 'ra_instance_eval_counts_map_f32')
    return inter, area_b, wmap
  check(rn.lib().ra_instance_eval_counts_f32(ptr(yc), ptr(gt_ids), ptr(inst_id), ptr(fg), B, T, Hs, Ws, Hf, Wf, int(bool(morph)),
                                             ptr(thr), K, ptr(inter), ptr(area_b), rn.stream_ptr()), 'ra_instance_eval_counts_f32')
  return inter, area_b


def eval_metrics_from_counts(inter, area_b, s_gt, remove_tiny=0, conf=None):
  """What eval_metrics returns — dict(iou_pairwise [B,T,T], stats [B,len(EVAL_NAMES)], inst [B,len(EVALI_NAMES),T], sizes
  [B,T]) — for every threshold of instance_eval_counts' (inter [B,K,T,T + 1], area_b [B,T]): a list of K dicts, from ONE
  ra_eval_metrics_f32 launch over the B * K problems.  remove_tiny (postprocess.py:109-136) acts on the counts: a prediction
  whose area is <= remove_tiny loses its row, and its entry of conf [B,T] (apply_confidence's s_out > 0.5) becomes 0; every
  dict then carries 'conf' [B,T].  The chain applies it only where a foreground was given (full_model_eval.py:121-124): pass 0
  otherwise.  The kernel's foreground terms are sums of the counts: the predictions are disjoint after apply_one_label and
  the instances of an id image are disjoint by construction, so the area of a union is the sum of the areas.  Every number
  is an integer below 2^24, exact in float32 in any order of summation."""
  if not all(isinstance(t, torch.Tensor) and t.is_cuda for t in (inter, area_b, s_gt)):
    raise rn.RecAttendError('eval_metrics_from_counts needs CUDA (HIP) tensors; got a CPU tensor. There is no CPU fallback.')
  if inter.dim() != 4 or inter.shape[3] != inter.shape[2] + 1 or tuple(area_b.shape) != (inter.shape[0], inter.shape[2]) or \
      tuple(s_gt.shape) != tuple(area_b.shape):
    raise rn.RecAttendError('eval_metrics_from_counts: inter must be [B,K,T,T + 1], area_b and s_gt [B,T], got %s, %s, %s' % (
        tuple(inter.shape), tuple(area_b.shape), tuple(s_gt.shape)))
  B, K, T, _ = inter.shape
  dev = inter.device
  cnt = inter.to(torch.float32)
  sum_a = cnt.sum(dim=3)  # [B,K,T]: the predictions' areas
  conf_k = None if conf is None else conf.to(torch.float32)[:, None, :].expand(B, K, T)
  if remove_tiny:
    keep = (sum_a > float(remove_tiny)).to(torch.float32)
    cnt, sum_a = cnt * keep[..., None], sum_a * keep
    conf_k = None if conf_k is None else conf_k * keep
  main = cnt[..., :T].reshape(B * K, T, T).contiguous()
  sum_a = sum_a.reshape(B * K, T).contiguous()
  sum_b = area_b.to(torch.float32)[:, None, :].expand(B, K, T).reshape(B * K, T).contiguous()
  sg = s_gt.to(torch.float32)[:, None, :].expand(B, K, T).reshape(B * K, T).contiguous()
  fg_inter, fg_a, fg_b = main.sum(dim=(1, 2)).contiguous(), sum_a.sum(dim=1).contiguous(), sum_b.sum(dim=1).contiguous()
  a_fgb, b_fga = main.sum(dim=2).contiguous(), main.sum(dim=1).contiguous()
  iou = torch.empty((B * K, T, T), dtype=torch.float32, device=dev)
  stats = torch.empty((B * K, len(EVAL_NAMES)), dtype=torch.float32, device=dev)
  inst = torch.empty((B * K, len(EVALI_NAMES), T), dtype=torch.float32, device=dev)
  check(rn.lib().ra_eval_metrics_f32(ptr(main), ptr(sum_a), ptr(sum_b), ptr(sg), ptr(fg_inter), ptr(fg_a), ptr(fg_b), ptr(a_fgb),
                                     ptr(b_fga), B * K, T, ptr(iou), ptr(stats), ptr(inst), rn.stream_ptr()), 'ra_eval_metrics_f32')
  iou, stats, inst, sum_a = (iou.view(B, K, T, T), stats.view(B, K, -1), inst.view(B, K, len(EVALI_NAMES), T), sum_a.view(B, K, T))
  out = []
  for k in range(K):
    d = {'iou_pairwise': iou[:, k], 'stats': stats[:, k], 'inst': inst[:, k], 'sizes': sum_a[:, k]}
    if conf_k is not None:
      d['conf'] = conf_k[:, k]
    out.append(d)
  return out


# ---------------------------------------------------------------------------- the label stage: ground truth from instance ids
LABELS_MAX_T = rn.RA_LABELS_MAX_T
LABEL_DATASETS = {'cvppp': rn.RA_LABELS_PLAIN, 'kitti': rn.RA_LABELS_PLAIN, 'plain': rn.RA_LABELS_PLAIN,
                  'cityscapes': rn.RA_LABELS_CITYSCAPES}
LABEL_OUTPUTS = ('num_obj', 's_gt', 'inst_id', 'area', 'sem_cls', 'y_gt', 'd_cls', 'd_gt', 'c_gt', 'fg_gt_full')


def label_dataset_rule(dataset):
  """RA_LABELS_* of a dataset name (cvppp, kitti: every id != 0 is an instance; cityscapes: labelId * 1000 + k of the eight
  instance labels) or of the constant itself."""
  if dataset in LABEL_DATASETS:
    return LABEL_DATASETS[dataset]
  if dataset in (rn.RA_LABELS_PLAIN, rn.RA_LABELS_CITYSCAPES) and not isinstance(dataset, bool):
    return int(dataset)
  raise rn.RecAttendError('assemble_labels: dataset %r (one of %s)' % (dataset, ', '.join(sorted(LABEL_DATASETS))))


def assemble_labels_raw(gt_ids, catalog, H, W, T, dataset, want=LABEL_OUTPUTS):
  """ra_labels_assemble_i32 on gt_ids int32 [B,Hf,Wf] and catalog = gt_instance_catalog(gt_ids, ...) of the same tensor:
  {name: device tensor} over `want`; no status is looked at."""
  _need_cuda_i32(gt_ids, 'gt_ids')
  ids, count = catalog[0], catalog[2]
  _need_cuda_i32(ids, 'catalog ids')
  _need_cuda_i32(count, 'catalog count')
  rule = label_dataset_rule(dataset)
  unknown = [k for k in want if k not in LABEL_OUTPUTS]
  if unknown or not want:
    raise rn.RecAttendError('assemble_labels: want %s (any of %s)' % (list(want), ', '.join(LABEL_OUTPUTS)))
  if gt_ids.dim() != 3 or min(gt_ids.shape) < 1:
    raise rn.RecAttendError('assemble_labels: gt_ids must be [B,Hf,Wf], got %s' % (tuple(gt_ids.shape),))
  B, Hf, Wf = gt_ids.shape
  H, W, T = int(H), int(W), int(T)
  if tuple(ids.shape) != (B, MAX_GT) or tuple(count.shape) != (B,):
    raise rn.RecAttendError('assemble_labels: gt_ids %s, catalog ids %s, count %s do not belong together' % (
        tuple(gt_ids.shape), tuple(ids.shape), tuple(count.shape)))
  if not (1 <= T <= LABELS_MAX_T and 1 <= H <= Hf and 1 <= W <= Wf and Hf * Wf < 1 << 31 and B <= OVERLAP_MAX_B):
    raise rn.RecAttendError('assemble_labels: T=%d, %d x %d -> %d x %d, B=%d (1 <= T <= %d, 1 <= H <= Hf, 1 <= W <= Wf, Hf * Wf < '
                            '2^31, B <= %d)' % (T, Hf, Wf, H, W, B, LABELS_MAX_T, OVERLAP_MAX_B))
  dev = gt_ids.device
  nc = 1 + len(_cityscapes_labels()) if rule == rn.RA_LABELS_CITYSCAPES else 1
  spec = {'num_obj': ((B,), torch.int32), 's_gt': ((B, T), torch.float32), 'inst_id': ((B, T), torch.int32),
          'area': ((B, T), torch.int32), 'sem_cls': ((B, T), torch.int32), 'y_gt': ((B, T, H, W), torch.float32),
          'd_cls': ((B, H, W), torch.uint8), 'd_gt': ((B, H, W, 8), torch.float32), 'c_gt': ((B, H, W, nc), torch.float32),
          'fg_gt_full': ((B, Hf, Wf), torch.uint8)}
  out = {k: torch.empty(spec[k][0], dtype=spec[k][1], device=dev) for k in LABEL_OUTPUTS if k in want}
  n = rn.lib().ra_labels_workspace_bytes(B, H, W)
  ws = torch.empty((max(n // 8, 1),), dtype=torch.int64, device=dev)
  check(rn.lib().ra_labels_assemble_i32(ptr(gt_ids), ptr(ids), ptr(count), B, Hf, Wf, H, W, T, rule, ptr(ws), n,
                                        *[ptr(out.get(k)) for k in LABEL_OUTPUTS], rn.stream_ptr()), 'ra_labels_assemble_i32')
  return out


def _cityscapes_labels():
  import analysis
  return analysis.CITYSCAPES_LABELS


def assemble_labels(gt_ids, H, W, T, dataset, want=('y_gt', 's_gt'), names=None):
  """The reference's label stage on the device (setup_*.py: ins_seg_assembler.py:85-155, read back by ins_seg_dataset.py:
  158-172,216-236,257-271): gt_ids [B,Hf,Wf] — a torch int32 tensor or a NumPy integer array of *_instanceIds.png values —
  -> {name: device tensor} over `want`, any of LABEL_OUTPUTS (include/recattend.h, ra_labels_assemble_i32, says what each
  is).  dataset: 'cvppp' | 'kitti' | 'cityscapes' or RA_LABELS_*.  Runs the catalogue of the full-size image and the
  stage's launches; an image with an id outside [0, 65535] or with more than MAX_GT distinct ids raises RecAttendError
  naming it (names[b], else its index), from one device-to-host copy of B status words."""
  if isinstance(gt_ids, np.ndarray):
    if not np.issubdtype(gt_ids.dtype, np.integer):
      raise rn.RecAttendError('assemble_labels: gt_ids must hold integers, got %s' % gt_ids.dtype)
    if not torch.cuda.is_available():
      raise rn.RecAttendError('recattend kernels need CUDA (HIP) tensors; no device is available. There is no CPU fallback.')
    gt_ids = torch.as_tensor(np.ascontiguousarray(gt_ids.astype(np.int32, copy=False))).cuda()
  label_dataset_rule(dataset)
  _need_cuda_i32(gt_ids, 'gt_ids')
  ids, pixels, count, status = gt_instance_catalog(gt_ids, check_status=False)
  out = assemble_labels_raw(gt_ids, (ids, pixels, count), H, W, T, dataset, want)
  _raise_gt_status(status, names, 'assemble_labels')
  return out


# ---- the image stage (csrc/ra_image.hip): x at network size from the full-size colour image
RESIZE_OUTPUTS = ('x', 'u8')
RESIZE_MAX_N = 65535  # images per launch (the grid's y extent)
_CUBIC_TABLES = {}    # (S, D, device) -> (ofs int32 [D], coef int16 [D,4]) on that device


def cubic_tables(S, D):
  """ra_resize_cubic_tables (host code, no device): one axis of cv2.resize(..., INTER_CUBIC) on 8-bit images, source length
  S -> destination length D, as include/recattend.h restates it -> (ofs int32 [D], coef int16 [D,4]) NumPy arrays: tap k of
  destination index d reads source index clamp(ofs[d] - 1 + k, 0, S - 1) with weight coef[d, k] / 2048."""
  S, D = int(S), int(D)
  ofs, coef = np.empty((max(D, 0),), np.int32), np.empty((max(D, 0), 4), np.int16)
  check(rn.lib().ra_resize_cubic_tables(S, D, ptr(ofs), ptr(coef)), 'ra_resize_cubic_tables')
  return ofs, coef


def _cubic_tables_dev(S, D, device):
  key = (S, D, str(device))
  if key not in _CUBIC_TABLES:
    ofs, coef = cubic_tables(S, D)
    _CUBIC_TABLES[key] = (torch.from_numpy(ofs).to(device), torch.from_numpy(coef).to(device))
  return _CUBIC_TABLES[key]


def resize_cubic(src, H, W, want=('x',)):
  """ins_seg_assembler.py:116 and ins_seg_dataset.py:149 on the device (ra_resize_cubic_u8): src uint8 [N,Hs,Ws,C], C = 1 | 3
  — a device tensor or a NumPy array — -> {'x': float32 [N,H,W,C] = level / 255, 'u8': uint8 [N,H,W,C]} over `want`.  The
  channel order is the caller's (cv2's BGR in the reference).  The tables of an (S, D) pair are made once per device."""
  want = tuple(want)
  if not want or any(k not in RESIZE_OUTPUTS for k in want):
    raise rn.RecAttendError('resize_cubic: want %s (any of %s)' % (list(want), ', '.join(RESIZE_OUTPUTS)))
  if isinstance(src, np.ndarray):
    if src.dtype != np.uint8:
      raise rn.RecAttendError('resize_cubic: src must be uint8, got %s' % src.dtype)
    if not torch.cuda.is_available():
      raise rn.RecAttendError('recattend kernels need CUDA (HIP) tensors; no device is available. There is no CPU fallback.')
    src = torch.from_numpy(np.ascontiguousarray(src)).cuda()
  _need_dev(src, torch.uint8, 'src')
  H, W = int(H), int(W)
  if src.dim() != 4 or min(src.shape) < 1 or src.shape[3] not in (1, 3) or H < 1 or W < 1:
    raise rn.RecAttendError('resize_cubic: src must be [N,Hs,Ws,C] with C = 1 or 3 and H, W >= 1, got %s -> %d x %d' % (
        tuple(src.shape), H, W))
  N, Hs, Ws, Cc = src.shape
  if N > RESIZE_MAX_N or Hs * Ws * Cc >= 1 << 31 or H * W * Cc * (4 if 'x' in want else 1) >= 1 << 31:
    raise rn.RecAttendError('resize_cubic: N=%d, %d x %d -> %d x %d, C=%d (N <= %d, every plane below 2^31 bytes)' % (
        N, Hs, Ws, H, W, Cc, RESIZE_MAX_N))
  dev = src.device
  oy, cy = _cubic_tables_dev(Hs, H, dev)
  ox, cx = _cubic_tables_dev(Ws, W, dev)
  out = {}
  if 'x' in want:
    out['x'] = torch.empty((N, H, W, Cc), dtype=torch.float32, device=dev)
  if 'u8' in want:
    out['u8'] = torch.empty((N, H, W, Cc), dtype=torch.uint8, device=dev)
  check(rn.lib().ra_resize_cubic_u8(ptr(src), N, Hs, Ws, Cc, H, W, ptr(oy), ptr(cy), ptr(ox), ptr(cx), ptr(out.get('u8')),
                                    ptr(out.get('x')), rn.stream_ptr()), 'ra_resize_cubic_u8')
  return out


# ---- the render stage (csrc/ra_render.hip): the colour images of analysis.py's render analyzers
RENDER_MAX_T = rn.RA_RENDER_MAX_T
RENDER_MIN_C, RENDER_MAX_C = 2, 16  # channels of d the orientation image takes
_RENDER_TABLES = {}                 # (what, T, device) -> uint8 table on that device


def _render_table(what, T, device):
  """The default colour tables, in the image's memory order (B, G, R): 'instances' — analysis.INSTANCE_CMAP[t % 22] reversed
  (the reference swaps its R, G, B image before cv2.imwrite) for t < T; 'wheel' — the first T rows of
  analysis.ORIENTATION_WHEEL as they stand (that array goes to cv2.imwrite unswapped)."""
  key = (what, T, str(device))
  if key not in _RENDER_TABLES:
    import analysis
    if what == 'instances':
      cmap = np.array(analysis.INSTANCE_CMAP, dtype=np.uint8)
      tab = cmap[np.arange(T) % cmap.shape[0]][:, ::-1]
    else:
      tab = np.array(analysis.ORIENTATION_WHEEL, dtype=np.uint8)[:T]
    _RENDER_TABLES[key] = torch.from_numpy(np.ascontiguousarray(tab)).to(device)
  return _RENDER_TABLES[key]


def render_instances(y, colours=None, first=False):
  """analysis.py:137-147 (first=False, RA_RENDER_ADD) / :166-187 (first=True, RA_RENDER_FIRST) on the device
  (ra_render_instances_u8): y float32 [B,T,H,W] with finite 0 <= y <= 255 -> uint8 [B,H,W,3] in the memory order cv2.imwrite
  takes (B, G, R; what utils/png.write_colour8 writes and read_colour8 reads).  Every plane is cast to uint8 and multiplied
  with its colour; the planes are summed in uint8 (both wrap), or with first=True laid UNDER what is there, decided per
  channel.  colours: uint8 [T,3] or [B,T,3] in the image's channel order (B, G, R); None = analysis.INSTANCE_CMAP[t % 22]
  as the file's R, G, B.  y is read once and not copied: a contiguous view at any offset is taken as it is."""
  _need_dev(y, torch.float32, 'y')
  if y.dim() != 4 or min(y.shape) < 1:
    raise rn.RecAttendError('render_instances: y must be [B,T,H,W], got %s' % (tuple(y.shape),))
  B, T, H, W = y.shape
  if T > RENDER_MAX_T or H * W > 1 << 30 or B > OVERLAP_MAX_B:
    raise rn.RecAttendError('render_instances: B=%d, T=%d, H * W = %d (B <= %d, T <= %d, H * W <= 2^30)' % (
        B, T, H * W, OVERLAP_MAX_B, RENDER_MAX_T))
  if colours is None:
    colours = _render_table('instances', T, y.device)
  _need_dev(colours, torch.uint8, 'colours')
  if tuple(colours.shape) == (T, 3):
    colours = colours.unsqueeze(0).expand(B, T, 3).contiguous()
  if tuple(colours.shape) != (B, T, 3):
    raise rn.RecAttendError('render_instances: colours must be [T,3] or [B,T,3] = [%d,%d,3], got %s' % (B, T, tuple(colours.shape)))
  img = torch.empty((B, H, W, 3), dtype=torch.uint8, device=y.device)
  check(rn.lib().ra_render_instances_u8(ptr(y), B, T, H, W, ptr(colours), rn.RA_RENDER_FIRST if first else rn.RA_RENDER_ADD,
                                        ptr(img), rn.stream_ptr()), 'ra_render_instances_u8')
  return img


def render_orientation(d, mask, size=None):
  """fg_model_eval.py:128-132,154-164 with data_api/orientation.py:13-28 on the device (ra_render_orientation_u8): d float32
  [B,Hs,Ws,C] at network size (2 <= C <= 8, the rows of analysis.ORIENTATION_WHEEL), mask float32 [B,H,W] of 0 / 1 at the
  labels' size (size, when given, must be its (H, W)) -> uint8 [B,H,W,3] in the memory order cv2.imwrite takes.  Every
  channel of d is resized with the linear resample of sem_labels inside the kernel, the first maximum is the class, the pixel
  its wheel row times the mask — written to a file as it stands, so the file's R, G, B is the wheel row reversed."""
  _need_dev(d, torch.float32, 'd')
  _need_dev(mask, torch.float32, 'mask')
  if d.dim() != 4 or mask.dim() != 3 or min(d.shape) < 1 or min(mask.shape) < 1 or mask.shape[0] != d.shape[0]:
    raise rn.RecAttendError('render_orientation: d must be [B,Hs,Ws,C] and mask [B,H,W], got %s and %s' % (
        tuple(d.shape), tuple(mask.shape)))
  B, Hs, Ws, Cc = d.shape
  H, W = int(mask.shape[1]), int(mask.shape[2])
  if size is not None and (int(size[0]), int(size[1])) != (H, W):
    raise rn.RecAttendError('render_orientation: size %s, but mask is %d x %d' % (tuple(size), H, W))
  wheel = _render_table('wheel', Cc, d.device)
  if not RENDER_MIN_C <= Cc <= min(RENDER_MAX_C, wheel.shape[0]) or wheel.shape[0] != Cc:
    raise rn.RecAttendError('render_orientation: d has %d channels (%d .. 8, the classes of the colour wheel)' % (Cc, RENDER_MIN_C))
  if H * W > 1 << 30 or Hs * Ws * Cc >= 1 << 31 or B > OVERLAP_MAX_B:
    raise rn.RecAttendError('render_orientation: B=%d, %d x %d x %d -> %d x %d (B <= %d, planes up to 2^30 pixels)' % (
        B, Hs, Ws, Cc, H, W, OVERLAP_MAX_B))
  img = torch.empty((B, H, W, 3), dtype=torch.uint8, device=d.device)
  check(rn.lib().ra_render_orientation_u8(ptr(d), B, Hs, Ws, Cc, ptr(mask), H, W, ptr(wheel), ptr(img), rn.stream_ptr()),
        'ra_render_orientation_u8')
  return img


# ------------------------------------------------------------- PNG output on the device (csrc/ra_png.hip)
_PNG_BUFFERS = {}  # device -> [workspace, out]: uint8 tensors that only grow, reused by every call on that device


PNG_CODES = {'fixed': 'ra_png_deflate', 'dynamic': 'ra_png_deflate_dyn'}  # the stream format -> its entry points' prefix


def _png_entry(who, code, suffix):
  """(the C entry point of the stream format `code`, its name)."""
  if code not in PNG_CODES:
    raise rn.RecAttendError("%s: code=%r (one of 'fixed', 'dynamic')" % (who, code))
  name = PNG_CODES[code] + suffix
  return getattr(rn.lib(), name), name


def png_deflate_bound(N, H, W, bpp, code='fixed'):
  """(bytes of one stream at most, bytes of workspace for N images) of ra_png_deflate_bound, or of ra_png_deflate_dyn_bound
  with code='dynamic'; bpp 1 (grey, float) or 3."""
  fn, name = _png_entry('png_deflate_bound', code, '_bound')
  stream, ws = C.c_ulonglong(0), C.c_ulonglong(0)
  check(fn(int(N), int(H), int(W), int(bpp), C.addressof(stream), C.addressof(ws)), name)
  return int(stream.value), int(ws.value)


def _png_source(who, src):
  """(kind, M, H, W, bpp) of a source tensor of png_deflate."""
  if not isinstance(src, torch.Tensor) or not src.is_contiguous():
    raise rn.RecAttendError('%s: src must be a contiguous tensor' % who)
  if src.dtype == torch.uint8 and src.dim() == 3:
    kind, bpp = rn.RA_PNG_GRAY8, 1
  elif src.dtype == torch.uint8 and src.dim() == 4 and src.shape[3] == 3:
    kind, bpp = rn.RA_PNG_BGR8, 3
  elif src.dtype == torch.float32 and src.dim() == 3:
    kind, bpp = rn.RA_PNG_F32, 1
  else:
    raise rn.RecAttendError('%s: src must be uint8 [N,H,W], uint8 [N,H,W,3] (B, G, R) or float32 [M,H,W], got %s %s' % (
        who, src.dtype, tuple(src.shape)))
  if min(src.shape) < 1:
    raise rn.RecAttendError('%s: src has an empty dimension: %s' % (who, tuple(src.shape)))
  return kind, int(src.shape[0]), int(src.shape[1]), int(src.shape[2]), bpp


def _png_planes(who, plane_index, M):
  """plane_index (a sequence or tensor of indices into the M source images) -> int32 NumPy array, checked on the host."""
  idx = plane_index.detach().cpu().numpy() if isinstance(plane_index, torch.Tensor) else np.asarray(plane_index)
  idx = idx.astype(np.int64).reshape(-1)
  if idx.size < 1 or idx.min() < 0 or idx.max() >= M:
    raise rn.RecAttendError('%s: plane_index must hold at least one index in [0, %d)' % (who, M))
  return np.ascontiguousarray(idx.astype(np.int32))


def png_deflate(src, plane_index=None, with_meta=False, code='fixed'):
  """The zlib streams of PNG image data (include/recattend.h, ra_png_deflate_u8: filter 0, one fixed-Huffman run-coded
  segment per scanline; code='dynamic': ra_png_deflate_dyn_u8, one dynamic-Huffman block per image, about a fifth of the bytes
  for a mask) for a batch of images on the device -> a list of bytes, one stream per image.  src: uint8 [N,H,W]
  (grey), uint8 [N,H,W,3] in B, G, R order (written as R, G, B) or float32 [M,H,W] quantised as (v * 255).to(uint8) for
  0 <= v <= 1.  plane_index: which source images to encode, in the order given (skipping, repeating and reordering are
  fine); None = all of them.  One launch chain, one small copy of the sizes and offsets, one copy of exactly the bytes used.
  with_meta: also return (sizes, offsets, adler) as the kernels wrote them, int64 / int64 / uint32 NumPy arrays [N]."""
  fn, name = _png_entry('png_deflate', code, '_u8')
  kind, M, H, W, bpp = _png_source('png_deflate', src)
  if not src.is_cuda:
    raise rn.RecAttendError('png_deflate: src must be on the device (png_deflate_host takes host arrays)')
  idx = None if plane_index is None else _png_planes('png_deflate', plane_index, M)
  N = M if idx is None else int(idx.size)
  stream, ws_bytes = png_deflate_bound(N, H, W, bpp, code)
  key = str(src.device)
  bufs = _PNG_BUFFERS.setdefault(key, [None, None])
  for k, need in enumerate((ws_bytes, N * stream)):
    if bufs[k] is None or bufs[k].numel() < need:
      bufs[k] = None
      bufs[k] = torch.empty((need,), dtype=torch.uint8, device=src.device)
  ws, out = bufs
  planes = None if idx is None else torch.from_numpy(idx).to(src.device)
  # sizes int32 [N], adler uint32 [N], offsets uint64 [N] in ONE tensor of 4 N words, so that one copy brings them back
  meta = torch.empty((4 * N,), dtype=torch.int32, device=src.device)
  check(fn(ptr(src), kind, M, N, H, W, ptr(planes), ptr(out), out.numel(), ptr(meta[:N]), ptr(meta[2 * N:]), ptr(meta[N:2 * N]),
           ptr(ws), ws.numel(), rn.stream_ptr()), name)
  host = meta.cpu().numpy()
  sizes, offsets = host[:N].astype(np.int64), host[2 * N:].view(np.int64)
  used = int(offsets[-1] + sizes[-1])
  data = out[:used].cpu().numpy().tobytes()
  streams = [data[int(o):int(o) + int(n)] for n, o in zip(sizes, offsets)]
  return (streams, sizes, offsets.copy(), host[N:2 * N].view(np.uint32).copy()) if with_meta else streams


def png_deflate_host(src, plane_index=None, code='fixed'):
  """png_deflate on host arrays through ra_png_deflate_host / ra_png_deflate_dyn_host (plain sequential C++, no GPU call): src a
  NumPy array of one of png_deflate's three kinds -> (list of streams, adler uint32 [N]).  What the device is compared with byte
  for byte."""
  fn, name = _png_entry('png_deflate_host', code, '_host')
  src = np.ascontiguousarray(src)
  kind, M, H, W, bpp = _png_source('png_deflate_host', torch.from_numpy(src))
  idx = None if plane_index is None else _png_planes('png_deflate_host', plane_index, M)
  N = M if idx is None else int(idx.size)
  stream, _ = png_deflate_bound(N, H, W, bpp, code)
  out = np.zeros((N * stream,), dtype=np.uint8)
  sizes, offsets, adler = np.zeros((N,), np.int32), np.zeros((N,), np.uint64), np.zeros((N,), np.uint32)
  check(fn(ptr(src), kind, M, N, H, W, ptr(idx), ptr(out), out.size, ptr(sizes), ptr(offsets), ptr(adler), None, 0), name)
  return [out[int(o):int(o) + int(n)].tobytes() for n, o in zip(sizes, offsets)], adler


def png_huffman_lengths(counts, limit=15):
  """ra_png_huffman_lengths (host code): the length-limited Huffman code lengths of the dynamic format's rule for a histogram
  of up to 286 counts, limit 7 or 15 -> uint8 [n]."""
  counts = np.ascontiguousarray(counts, dtype=np.uint32).reshape(-1)
  lengths = np.zeros((counts.size,), np.uint8)
  check(rn.lib().ra_png_huffman_lengths(ptr(counts), int(counts.size), int(limit), ptr(lengths)), 'ra_png_huffman_lengths')
  return lengths


# ------------------------------------------------------------- mixed full sizes in one batch (KITTI): the ragged entry points
# A batch of full-size images of different sizes is ONE flat tensor per per-pixel quantity plus its geometry: an int64 NumPy
# array [B,3] of (offset, h, w) rows on the host — image b is the h x w rows, packed with pitch w, from element `offset` on
# (include/recattend.h, ra_image_geo).
RAGGED_ALIGN = 4  # elements: pack_ragged starts every image at a multiple, so that real data takes the kernels' wide loads


def ragged_geometry(sizes, align=RAGGED_ALIGN):
  """The geometry [B,3] int64 of images of the given (h, w) sizes laid out in that order, each at the next multiple of
  `align` elements (align=1: no padding), and the flat buffer's element count."""
  geo = np.zeros((len(sizes), 3), dtype=np.int64)
  end = 0
  for b, (h, w) in enumerate(sizes):
    if int(h) < 1 or int(w) < 1:
      raise rn.RecAttendError('ragged_geometry: image %d is %d x %d (h, w >= 1)' % (b, h, w))
    start = -(-end // int(align)) * int(align)
    geo[b] = (start, int(h), int(w))
    end = start + int(h) * int(w)
  return geo, int(end)


def pack_ragged(arrays, dtype, device='cuda', align=RAGGED_ALIGN):
  """A list of [h,w] arrays (NumPy or torch) -> (flat tensor of `dtype` on `device`, geometry [B,3]): every image starts at a
  multiple of `align` elements, rows packed with pitch w, the gaps zero."""
  if not len(arrays) or any(getattr(a, 'ndim', 0) != 2 for a in arrays):
    raise rn.RecAttendError('pack_ragged: a non-empty list of [h,w] arrays')
  geo, total = ragged_geometry([tuple(a.shape) for a in arrays], align)
  flat = torch.zeros((total,), dtype=dtype)
  for (off, h, w), a in zip(geo.tolist(), arrays):
    a = a.detach().cpu() if isinstance(a, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(a))
    flat[off:off + h * w] = a.reshape(-1).to(dtype)
  return flat.to(device), geo


def unpack_ragged(flat, geo):
  """The images of a flat tensor as a list of [h,w] views."""
  return [flat[off:off + h * w].view(h, w) for off, h, w in np.asarray(geo).tolist()]


def _geo_table(who, geo, flat_tensors, device):
  """(ctypes table, device buffer, B, total) of a geometry [B,3] for flat tensors of one element count."""
  g = np.asarray(geo)
  if g.ndim != 2 or g.shape[1] != 3 or g.shape[0] < 1 or not np.issubdtype(g.dtype, np.integer):
    raise rn.RecAttendError('%s: geometry must be an integer array [B,3] of (offset, h, w), got %s %s' % (who, g.dtype, g.shape))
  B = int(g.shape[0])
  if B > OVERLAP_MAX_B:
    raise rn.RecAttendError('%s: B=%d (B <= %d)' % (who, B, OVERLAP_MAX_B))
  if np.abs(g[:, 1:]).max() >= 1 << 31:
    raise rn.RecAttendError('%s: geometry holds a size beyond 2^31' % who)
  total = int(flat_tensors[0].numel())
  for t in flat_tensors:
    if t.dim() != 1 or int(t.numel()) != total:
      raise rn.RecAttendError('%s: the flat tensors must be one-dimensional and of one length, got %s' % (
          who, [tuple(t.shape) for t in flat_tensors]))
  tab = (rn.ImageGeo * B)(*[rn.ImageGeo(int(o), int(h), int(w)) for o, h, w in g.tolist()])
  dev = torch.empty((B * C.sizeof(rn.ImageGeo) // 8,), dtype=torch.int64, device=device)
  return tab, dev, B, total


def gt_instance_catalog_ragged(gt_flat, geo, check_status=True, names=None):
  """gt_instance_catalog for a ragged batch: gt_flat int32 [P] and its geometry [B,3] -> (ids, pixels, count) as there, one
  catalogue per image (ra_gt_instance_catalog_ragged_i32).  check_status=False returns the status words as a fourth tensor."""
  _need_cuda_i32(gt_flat, 'gt_flat')
  tab, gdev, B, total = _geo_table('gt_instance_catalog_ragged', geo, (gt_flat,), gt_flat.device)
  dev = gt_flat.device
  n = rn.lib().ra_gt_instance_catalog_ragged_workspace_ints(tab, B)
  ws = torch.empty((max(n, 1),), dtype=torch.int32, device=dev)
  ids = torch.empty((B, MAX_GT), dtype=torch.int32, device=dev)
  pixels = torch.empty((B, MAX_GT), dtype=torch.int32, device=dev)
  count = torch.empty((B,), dtype=torch.int32, device=dev)
  status = torch.empty((B,), dtype=torch.int32, device=dev)
  check(rn.lib().ra_gt_instance_catalog_ragged_i32(ptr(gt_flat), total, tab, ptr(gdev), B, ptr(ws), n, ptr(ids), ptr(pixels),
                                                   ptr(count), ptr(status), rn.stream_ptr()), 'ra_gt_instance_catalog_ragged_i32')
  if not check_status:
    return ids, pixels, count, status
  _raise_gt_status(status, names, 'gt_instance_catalog_ragged')
  return ids, pixels, count


def assemble_labels_ragged_raw(gt_flat, geo, catalog, H, W, T, dataset, want=LABEL_OUTPUTS):
  """ra_labels_assemble_ragged_i32 on gt_flat int32 [P], its geometry and catalog = gt_instance_catalog_ragged(gt_flat, geo,
  ...): {name: device tensor} over `want` — the network-size outputs dense as assemble_labels_raw has them, 'fg_gt_full' uint8
  [P] flat at gt_flat's offsets (the gaps between images zero); no status is looked at."""
  who = 'assemble_labels_ragged'
  _need_cuda_i32(gt_flat, 'gt_flat')
  ids, count = catalog[0], catalog[2]
  _need_cuda_i32(ids, 'catalog ids')
  _need_cuda_i32(count, 'catalog count')
  rule = label_dataset_rule(dataset)
  unknown = [k for k in want if k not in LABEL_OUTPUTS]
  if unknown or not want:
    raise rn.RecAttendError('%s: want %s (any of %s)' % (who, list(want), ', '.join(LABEL_OUTPUTS)))
  tab, gdev, B, total = _geo_table(who, geo, (gt_flat,), gt_flat.device)
  H, W, T = int(H), int(W), int(T)
  if tuple(ids.shape) != (B, MAX_GT) or tuple(count.shape) != (B,):
    raise rn.RecAttendError('%s: %d images, catalog ids %s, count %s do not belong together' % (
        who, B, tuple(ids.shape), tuple(count.shape)))
  if not (1 <= T <= LABELS_MAX_T and H >= 1 and W >= 1 and H * W < 1 << 31):
    raise rn.RecAttendError('%s: T=%d -> %d x %d (1 <= T <= %d, H, W >= 1, H * W < 2^31)' % (who, T, H, W, LABELS_MAX_T))
  dev = gt_flat.device
  nc = 1 + len(_cityscapes_labels()) if rule == rn.RA_LABELS_CITYSCAPES else 1
  spec = {'num_obj': ((B,), torch.int32), 's_gt': ((B, T), torch.float32), 'inst_id': ((B, T), torch.int32),
          'area': ((B, T), torch.int32), 'sem_cls': ((B, T), torch.int32), 'y_gt': ((B, T, H, W), torch.float32),
          'd_cls': ((B, H, W), torch.uint8), 'd_gt': ((B, H, W, 8), torch.float32), 'c_gt': ((B, H, W, nc), torch.float32)}
  out = {k: torch.empty(spec[k][0], dtype=spec[k][1], device=dev) for k in LABEL_OUTPUTS if k in want and k in spec}
  if 'fg_gt_full' in want:
    out['fg_gt_full'] = torch.zeros((total,), dtype=torch.uint8, device=dev)
  n = rn.lib().ra_labels_workspace_bytes(B, H, W)
  ws = torch.empty((max(n // 8, 1),), dtype=torch.int64, device=dev)
  check(rn.lib().ra_labels_assemble_ragged_i32(ptr(gt_flat), total, tab, ptr(gdev), ptr(ids), ptr(count), B, H, W, T, rule, ptr(ws),
                                               n, *[ptr(out.get(k)) for k in LABEL_OUTPUTS], rn.stream_ptr()),
        'ra_labels_assemble_ragged_i32')
  return out


def assemble_labels_ragged(gt_flat, geo, H, W, T, dataset, want=('y_gt', 's_gt'), names=None):
  """assemble_labels for a ragged batch (KITTI's mixed full sizes): gt_flat int32 [P] on the device with its geometry [B,3] (what
  pack_ragged returns) -> {name: device tensor} over `want`.  The network-size outputs are dense ([B,T,H,W] and the like), the
  nearest-neighbour sampling scale is each image's own, and 'fg_gt_full' is flat at gt_flat's offsets.  1 <= H <= h and 1 <= W <=
  w must hold for every image.  Status words as in assemble_labels."""
  label_dataset_rule(dataset)
  _need_cuda_i32(gt_flat, 'gt_flat')
  ids, pixels, count, status = gt_instance_catalog_ragged(gt_flat, geo, check_status=False)
  out = assemble_labels_ragged_raw(gt_flat, geo, (ids, pixels, count), H, W, T, dataset, want)
  _raise_gt_status(status, names, 'assemble_labels_ragged')
  return out


def instance_eval_counts_ragged(yc, gt_flat, geo, inst_id, thresholds, fg_flat=None, morph=False, check_fg=True, want_map=False,
                                map_out=None):
  """instance_eval_counts for a ragged batch: yc float32 [B,T,Hs,Ws] and inst_id int32 [B,T] dense, gt_flat int32 [P] and
  fg_flat uint8 [P] (or None) flat with one geometry [B,3] -> (inter int32 [B,K,T,T + 1], area_b int32 [B,T]) as there; every
  image is resized, filtered and walked at its own h x w, h * w <= 2^24 (ra_instance_eval_counts_ragged_f32).  want_map: and
  the winner map uint16 [P], flat at gt_flat's offsets (ra_instance_eval_counts_map_ragged_f32); the elements between the
  images are zero in a map made here and left as they are in map_out."""
  who = 'instance_eval_counts_ragged'
  thr = _ins_eval_thresholds(thresholds)
  ts = (yc, gt_flat, inst_id) + (() if fg_flat is None else (fg_flat,))
  if not all(isinstance(t, torch.Tensor) for t in ts) or not all(t.is_cuda for t in ts):
    raise rn.RecAttendError('%s needs CUDA (HIP) tensors; got a CPU tensor. There is no CPU fallback.' % who)
  if yc.dtype != torch.float32 or gt_flat.dtype != torch.int32 or inst_id.dtype != torch.int32 or not all(t.is_contiguous() for t in ts):
    raise rn.RecAttendError('%s: yc must be contiguous float32, gt_flat and inst_id contiguous int32, got %s, %s, %s' % (
        who, yc.dtype, gt_flat.dtype, inst_id.dtype))
  if fg_flat is not None and fg_flat.dtype != torch.uint8:
    raise rn.RecAttendError('%s: fg_flat must be uint8, got %s' % (who, fg_flat.dtype))
  tab, gdev, B, total = _geo_table(who, geo, (gt_flat,) + (() if fg_flat is None else (fg_flat,)), yc.device)
  if yc.dim() != 4 or min(yc.shape) < 1 or yc.shape[0] != B or tuple(inst_id.shape) != tuple(yc.shape[:2]):
    raise rn.RecAttendError('%s: yc must be [B,T,Hs,Ws] and inst_id [B,T] for the geometry\'s %d images, got %s, %s' % (
        who, B, tuple(yc.shape), tuple(inst_id.shape)))
  _, T, Hs, Ws = yc.shape
  if not (T <= LABELS_MAX_T and Hs * Ws < 1 << 31):
    raise rn.RecAttendError('%s: T=%d, %d x %d (T <= %d, Hs * Ws < 2^31)' % (who, T, Hs, Ws, LABELS_MAX_T))
  if fg_flat is not None and check_fg and int(fg_flat.max()) > 1:
    raise rn.RecAttendError('%s: fg_flat holds %d; a foreground mask is 0 / 1' % (who, int(fg_flat.max())))
  K = int(thr.size)
  inter = torch.empty((B, K, T, T + 1), dtype=torch.int32, device=yc.device)
  area_b = torch.empty((B, T), dtype=torch.int32, device=yc.device)
  if want_map or map_out is not None:
    # the kernel never writes between the images: a new map starts as zeros, so that what it holds there is no stale memory
    wmap = torch.zeros((total,), dtype=torch.uint16, device=yc.device) if map_out is None else _ins_eval_map(who, map_out, (total,), yc.device)
    check(rn.lib().ra_instance_eval_counts_map_ragged_f32(ptr(yc), ptr(gt_flat), ptr(inst_id), ptr(fg_flat), total, tab, ptr(gdev),
                                                          B, T, Hs, Ws, int(bool(morph)), ptr(thr), K, ptr(inter), ptr(area_b),
                                                          ptr(wmap), rn.stream_ptr()), 'ra_instance_eval_counts_map_ragged_f32')
    return inter, area_b, wmap
  check(rn.lib().ra_instance_eval_counts_ragged_f32(ptr(yc), ptr(gt_flat), ptr(inst_id), ptr(fg_flat), total, tab, ptr(gdev), B, T,
                                                    Hs, Ws, int(bool(morph)), ptr(thr), K, ptr(inter), ptr(area_b),
                                                    rn.stream_ptr()), 'ra_instance_eval_counts_ragged_f32')
  return inter, area_b


def fg_sweep_counts_ragged_device(src, gt_flat, geo, thresholds, out=None):
  """ra_fg_sweep_counts_ragged_f32 without the copy to the host: src float32 [N,Hs,Ws], gt_flat uint8 [P] with its geometry
  [N,3] -> int64 device tensor [N, RA_FG_SWEEP_SLOTS] as fg_sweep_counts_device returns it."""
  who = 'fg_sweep_counts_ragged'
  thr = _sweep_thresholds(thresholds)
  if not (isinstance(src, torch.Tensor) and isinstance(gt_flat, torch.Tensor)) or not src.is_cuda or not gt_flat.is_cuda:
    raise rn.RecAttendError('%s needs CUDA (HIP) tensors; got a CPU tensor. There is no CPU fallback.' % who)
  if src.dtype != torch.float32 or gt_flat.dtype != torch.uint8 or not src.is_contiguous() or not gt_flat.is_contiguous():
    raise rn.RecAttendError('%s: src must be contiguous float32 and gt_flat contiguous uint8, got %s and %s' % (
        who, src.dtype, gt_flat.dtype))
  tab, gdev, N, total = _geo_table(who, geo, (gt_flat,), src.device)
  if src.dim() != 3 or min(src.shape) < 1 or src.shape[0] != N:
    raise rn.RecAttendError('%s: src must be [N,Hs,Ws] for the geometry\'s %d images, got %s' % (who, N, tuple(src.shape)))
  _, Hs, Ws = src.shape
  if Hs * Ws >= 1 << 31:
    raise rn.RecAttendError('%s: %d x %d (planes below 2^31 pixels)' % (who, Hs, Ws))
  if out is None:
    out = torch.empty((N, rn.RA_FG_SWEEP_SLOTS), dtype=torch.int64, device=src.device)
  elif tuple(out.shape) != (N, rn.RA_FG_SWEEP_SLOTS) or out.dtype != torch.int64 or not out.is_cuda or not out.is_contiguous():
    raise rn.RecAttendError('%s: out must be a contiguous int64 device tensor [%d, %d]' % (who, N, rn.RA_FG_SWEEP_SLOTS))
  check(rn.lib().ra_fg_sweep_counts_ragged_f32(ptr(src), ptr(gt_flat), total, tab, ptr(gdev), N, Hs, Ws, ptr(thr), int(thr.size),
                                               ptr(out), rn.stream_ptr()), 'ra_fg_sweep_counts_ragged_f32')
  return out


def fg_sweep_counts_ragged(src, gt_flat, geo, thresholds):
  """fg_sweep_counts for a ragged batch -> {'count_a' [N,K], 'sum_ab' [N,K], 'sum_b' [N], 'pixels' [N] (h * w PER IMAGE),
  'thresholds'}: NumPy int64 on the host."""
  c = fg_sweep_counts_ragged_device(src, gt_flat, geo, thresholds).cpu().numpy()
  K = len(_sweep_thresholds(thresholds))
  g = np.asarray(geo, dtype=np.int64)
  return {'count_a': c[:, :K].copy(), 'sum_ab': c[:, FG_SWEEP_MAX_K:FG_SWEEP_MAX_K + K].copy(), 'sum_b': c[:, 2 * FG_SWEEP_MAX_K].copy(),
          'pixels': (g[:, 1] * g[:, 2]).copy(), 'thresholds': [float(t) for t in _sweep_thresholds(thresholds)]}


# ------------------------------------------ pictures on the id path: paint from the winner map (csrc/ra_instance_paint.hip)
def _paint_geometry(who, t, dtype, what, geo):
  """(table, device table, B, total, shape of one picture) of a uniform [B,Hf,Wf] or, with geo, a flat [P] device tensor."""
  if not isinstance(t, torch.Tensor) or not t.is_cuda:
    raise rn.RecAttendError('%s needs CUDA (HIP) tensors; got a CPU tensor. There is no CPU fallback.' % who)
  if t.dtype != dtype or not t.is_contiguous():
    raise rn.RecAttendError('%s: %s must be contiguous %s, got %s' % (who, what, dtype, t.dtype))
  if geo is None:
    if t.dim() != 3 or min(t.shape) < 1:
      raise rn.RecAttendError('%s: %s must be [B,Hf,Wf] (or flat [P] with its geometry), got %s' % (who, what, tuple(t.shape)))
    B, Hf, Wf = (int(n) for n in t.shape)
    if Hf * Wf > INS_EVAL_MAX_PIXELS or B > OVERLAP_MAX_B:
      raise rn.RecAttendError('%s: B=%d, %d x %d (B <= %d, Hf * Wf <= 2^24)' % (who, B, Hf, Wf, OVERLAP_MAX_B))
    return None, None, B, B * Hf * Wf, (B, Hf, Wf)
  if t.dim() != 1:
    raise rn.RecAttendError('%s: with a geometry %s must be flat [P], got %s' % (who, what, tuple(t.shape)))
  tab, gdev, B, total = _geo_table(who, geo, (t,), t.device)
  return tab, gdev, B, total, (total,)


def _paint_colours(who, colours, lead, T, device):
  """colours uint8 [T,3] or lead + [T,3] (or a suffix of lead in front of [T,3]) -> contiguous lead + [T,3] on the device."""
  _need_dev(colours, torch.uint8, 'colours')
  shape = tuple(colours.shape)
  if colours.dim() < 2 or colours.dim() > len(lead) + 2 or shape[-2:] != (T, 3) or \
      (colours.dim() > 2 and shape[:-2] != tuple(lead)[:colours.dim() - 2]):
    raise rn.RecAttendError('%s: colours must be [T,3] or %s = %s, got %s' % (
        who, ' / '.join('[%s,T,3]' % ','.join('BK'[:n]) for n in range(1, len(lead) + 1)), list(lead) + [T, 3], shape))
  while colours.dim() < len(lead) + 2:  # [T,3] -> [1,T,3]; [B,T,3] -> [B,1,T,3]
    colours = colours.unsqueeze(0 if colours.dim() == 2 else colours.dim() - 2)
  return colours.expand(*lead, T, 3).contiguous()


def paint_keep(per_threshold):
  """keep bool [B,K,T] for paint_instances from the list eval_metrics_from_counts returns: a prediction is painted at
  threshold k iff the metrics of that threshold count it (its 'sizes' entry is not zero: remove_tiny zeroes it there)."""
  return torch.stack([d['sizes'] > 0 for d in per_threshold], dim=1)


def paint_instances(wmap, thresholds, colours=None, keep=None, geo=None, out=None):
  """analysis.py:137-147 on the id path (ra_instance_paint_u8 / ra_instance_paint_ragged_u8): the winner map of
  instance_eval_counts(..., want_map=True) — uint16 [B,Hf,Wf], or flat [P] with its geometry `geo` — and `thresholds`, THE list of
  that call (the map counts ranks among them) -> uint8 [Kp,B,Hf,Wf,3] (flat: [Kp,P,3], image b of picture k at
  out[k, offset_b : offset_b + h * w]), one picture per threshold, in the order given, in the memory order
  utils/png.write_colour8 takes (B, G, R): colour[t*] where the pixel passes the threshold, black elsewhere.  colours: uint8 [T,3], [B,T,3] or [B,Kp,T,3]; None = analysis.INSTANCE_CMAP[t % 22] for 32 predictions.
  keep: bool [B,Kp,T] (paint_keep), False = that prediction is not painted in that picture (remove_tiny).  Elements between the
  images of a flat batch are zero in a result made here and left as they are in `out`."""
  who = 'paint_instances'
  pos = ins_eval_threshold_pos(thresholds)
  Kp = int(pos.size)
  tab, gdev, B, total, shape = _paint_geometry(who, wmap, torch.uint16, 'map', geo)
  dev = wmap.device
  if colours is not None:
    T = int(colours.shape[-2]) if isinstance(colours, torch.Tensor) and colours.dim() >= 2 else 0
  elif keep is not None:
    T = int(keep.shape[-1]) if isinstance(keep, torch.Tensor) and keep.dim() == 3 else 0
  else:
    T = LABELS_MAX_T
  if not 1 <= T <= LABELS_MAX_T:
    raise rn.RecAttendError('%s: T=%d (1 <= T <= %d)' % (who, T, LABELS_MAX_T))
  if colours is None:
    colours = _render_table('instances', T, dev)
  colours = _paint_colours(who, colours, (B, Kp), T, dev)
  if keep is not None:
    if not isinstance(keep, torch.Tensor) or not keep.is_cuda or keep.dtype != torch.bool or tuple(keep.shape) != (B, Kp, T):
      raise rn.RecAttendError('%s: keep must be a bool device tensor [B,Kp,T] = [%d,%d,%d]' % (who, B, Kp, T))
    colours = (colours * keep[..., None].to(torch.uint8)).contiguous()
  want = (Kp,) + shape + (3,)
  if out is None:
    out = torch.empty(want, dtype=torch.uint8, device=dev) if geo is None else torch.zeros(want, dtype=torch.uint8, device=dev)
  elif not isinstance(out, torch.Tensor) or not out.is_cuda or out.dtype != torch.uint8 or tuple(out.shape) != want or not out.is_contiguous():
    raise rn.RecAttendError('%s: out must be a contiguous uint8 device tensor %s' % (who, want))
  if geo is None:
    check(rn.lib().ra_instance_paint_u8(ptr(wmap), B, shape[1], shape[2], ptr(pos), Kp, T, ptr(colours), ptr(out), rn.stream_ptr()),
          'ra_instance_paint_u8')
  else:
    check(rn.lib().ra_instance_paint_ragged_u8(ptr(wmap), total, tab, ptr(gdev), B, ptr(pos), Kp, T, ptr(colours), ptr(out),
                                               rn.stream_ptr()), 'ra_instance_paint_ragged_u8')
  return out


def paint_groundtruth(gt_ids, inst_id, colours, geo=None, out=None):
  """analysis.py:166-187 on the id path (ra_gt_paint_u8 / ra_gt_paint_ragged_u8): gt_ids int32 [B,Hf,Wf], or flat [P] with its
  geometry; inst_id int32 [B,T] (the id of ground-truth slot j, negative = empty); colours uint8 [T,3] or [B,T,3] in the
  picture's channel order (B, G, R) -> uint8 [B,Hf,Wf,3] ([P,3]): the colour of the first slot that lists the pixel's id,
  black where none does — render_instances(gt planes, colours, first=True) without the planes."""
  who = 'paint_groundtruth'
  tab, gdev, B, total, shape = _paint_geometry(who, gt_ids, torch.int32, 'gt_ids', geo)
  _need_cuda_i32(inst_id, 'inst_id')
  if inst_id.dim() != 2 or inst_id.shape[0] != B or not 1 <= inst_id.shape[1] <= LABELS_MAX_T:
    raise rn.RecAttendError('%s: inst_id must be [B,T] = [%d, 1 .. %d], got %s' % (who, B, LABELS_MAX_T, tuple(inst_id.shape)))
  T = int(inst_id.shape[1])
  colours = _paint_colours(who, colours, (B,), T, gt_ids.device)
  want = shape + (3,)
  if out is None:
    out = torch.empty(want, dtype=torch.uint8, device=gt_ids.device) if geo is None else torch.zeros(want, dtype=torch.uint8, device=gt_ids.device)
  elif not isinstance(out, torch.Tensor) or not out.is_cuda or out.dtype != torch.uint8 or tuple(out.shape) != want or not out.is_contiguous():
    raise rn.RecAttendError('%s: out must be a contiguous uint8 device tensor %s' % (who, want))
  if geo is None:
    check(rn.lib().ra_gt_paint_u8(ptr(gt_ids), ptr(inst_id), B, T, shape[1], shape[2], ptr(colours), ptr(out), rn.stream_ptr()),
          'ra_gt_paint_u8')
  else:
    check(rn.lib().ra_gt_paint_ragged_u8(ptr(gt_ids), total, tab, ptr(gdev), ptr(inst_id), B, T, ptr(colours), ptr(out),
                                         rn.stream_ptr()), 'ra_gt_paint_ragged_u8')
  return out


# ------------------------------------- PNG output of a ragged batch: one launch chain for mixed sizes (csrc/ra_png.hip, ra_png_dyn.hip)
def _png_ragged_source(who, src):
  """(kind, M, P, bpp) of a source of png_deflate_ragged: uint8 [M,P], uint8 [M,P,3] (B, G, R) or float32 [M,P]; a one-plane
  uint8 [P,3] or, of either type, [P] is M = 1."""
  if not isinstance(src, torch.Tensor) or not src.is_contiguous():
    raise rn.RecAttendError('%s: src must be a contiguous tensor' % who)
  shape = tuple(int(n) for n in src.shape)
  if src.dtype == torch.uint8 and len(shape) in (2, 3) and shape[-1] == 3:  # a two-dimensional [n,3] is ONE colour plane
    kind, bpp, lead = rn.RA_PNG_BGR8, 3, shape[:-1]
  elif src.dtype == torch.uint8 and len(shape) in (1, 2):
    kind, bpp, lead = rn.RA_PNG_GRAY8, 1, shape
  elif src.dtype == torch.float32 and len(shape) in (1, 2):
    kind, bpp, lead = rn.RA_PNG_F32, 1, shape
  else:
    raise rn.RecAttendError('%s: src must be uint8 [M,P], uint8 [M,P,3] (B, G, R) or float32 [M,P] (one plane: [P], [P,3]), '
                            'got %s %s' % (who, src.dtype, shape))
  M, P = (1, lead[0]) if len(lead) == 1 else lead
  if M < 1 or P < 1:
    raise rn.RecAttendError('%s: src has an empty dimension: %s' % (who, shape))
  return kind, M, P, bpp


def png_deflate_ragged_bound(geo, Np, bpp, code='fixed'):
  """(bytes of all Np * B streams at most — Np times the sum of the images' own bounds —, bytes of workspace) of
  ra_png_deflate_ragged_bound, or of ra_png_deflate_dyn_ragged_bound with code='dynamic'; geo: the geometry [B,3], bpp 1 or 3."""
  fn, name = _png_entry('png_deflate_ragged_bound', code, '_ragged_bound')
  tab, _, B, _ = _geo_table('png_deflate_ragged_bound', geo, (torch.empty((0,)),), 'cpu')
  out, ws = C.c_ulonglong(0), C.c_ulonglong(0)
  check(fn(tab, B, int(Np), int(bpp), C.addressof(out), C.addressof(ws)), name)
  return int(out.value), int(ws.value)


def png_deflate_ragged(src, geo, plane_index=None, with_meta=False, code='fixed'):
  """png_deflate for a batch of MIXED sizes in one launch chain (ra_png_deflate_ragged_u8 / ra_png_deflate_dyn_ragged_u8): src is
  M planes of P elements on the device — uint8 [M,P], uint8 [M,P,3] in B, G, R order (what paint_instances(..., geo=...) writes)
  or float32 [M,P]; [P] / [P,3] is one plane — all laid out by the geometry `geo` [B,3].  -> a list of Np * B streams, stream
  k * B + b = image b of plane plane_index[k] (None: of plane k, all M planes); every stream holds the bytes png_deflate gives
  for that image alone.  One copy of the metadata, one copy of exactly the bytes used.  with_meta: as png_deflate."""
  who = 'png_deflate_ragged'
  fn, name = _png_entry(who, code, '_ragged_u8')
  kind, M, P, bpp = _png_ragged_source(who, src)
  if not src.is_cuda:
    raise rn.RecAttendError('%s: src must be on the device (png_deflate_ragged_host takes host arrays)' % who)
  tab, gdev, B, total = _geo_table(who, geo, (src.view(-1)[:P],), src.device)
  idx = None if plane_index is None else _png_planes(who, plane_index, M)
  Np = M if idx is None else int(idx.size)
  N = Np * B
  out_bytes, ws_bytes = png_deflate_ragged_bound(geo, Np, bpp, code)
  bufs = _PNG_BUFFERS.setdefault(str(src.device), [None, None])
  for k, need in enumerate((ws_bytes, out_bytes)):
    if bufs[k] is None or bufs[k].numel() < need:
      bufs[k] = None
      bufs[k] = torch.empty((need,), dtype=torch.uint8, device=src.device)
  ws, out = bufs
  planes = None if idx is None else torch.from_numpy(idx).to(src.device)
  # sizes int32 [N], adler uint32 [N], offsets uint64 [N] in ONE tensor of 4 N words, so that one copy brings them back
  meta = torch.empty((4 * N,), dtype=torch.int32, device=src.device)
  check(fn(ptr(src), kind, M, total, tab, ptr(gdev), B, ptr(planes), Np, ptr(out), out.numel(), ptr(meta[:N]), ptr(meta[2 * N:]),
           ptr(meta[N:2 * N]), ptr(ws), ws.numel(), rn.stream_ptr()), name)
  host = meta.cpu().numpy()
  sizes, offsets = host[:N].astype(np.int64), host[2 * N:].view(np.int64)
  used = int(offsets[-1] + sizes[-1])
  data = out[:used].cpu().numpy().tobytes()
  streams = [data[int(o):int(o) + int(n)] for n, o in zip(sizes, offsets)]
  return (streams, sizes, offsets.copy(), host[N:2 * N].view(np.uint32).copy()) if with_meta else streams


def png_deflate_ragged_host(src, geo, plane_index=None, code='fixed'):
  """png_deflate_ragged on host arrays through ra_png_deflate_ragged_host / ra_png_deflate_dyn_ragged_host (plain sequential C++,
  no GPU call): src a NumPy array of one of png_deflate_ragged's kinds -> (list of streams, sizes int32 [N], offsets uint64 [N],
  adler uint32 [N])."""
  who = 'png_deflate_ragged_host'
  fn, name = _png_entry(who, code, '_ragged_host')
  src = np.ascontiguousarray(src)
  t = torch.from_numpy(src)
  kind, M, P, bpp = _png_ragged_source(who, t)
  tab, _, B, total = _geo_table(who, geo, (t.view(-1)[:P],), 'cpu')
  idx = None if plane_index is None else _png_planes(who, plane_index, M)
  Np = M if idx is None else int(idx.size)
  N = Np * B
  out_bytes, _ = png_deflate_ragged_bound(geo, Np, bpp, code)
  out = np.zeros((out_bytes,), dtype=np.uint8)
  sizes, offsets, adler = np.zeros((N,), np.int32), np.zeros((N,), np.uint64), np.zeros((N,), np.uint32)
  check(fn(ptr(src), kind, M, total, tab, B, ptr(idx), Np, ptr(out), out.size, ptr(sizes), ptr(offsets), ptr(adler), None, 0), name)
  return [out[int(o):int(o) + int(n)].tobytes() for n, o in zip(sizes, offsets)], sizes, offsets, adler
