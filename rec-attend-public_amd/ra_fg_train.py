"""Training the pre-stage fg_model (fg_model.py:94-266 of the reference): `FgTrainStep(model)` is to `fg_model.Model` what
`ra_train.TrainStep(model)` is to `full_model`.  By default for nets whose layers have up to 128 output channels; with
`FgTrainStep(model, wide=True)` also the nets the reference's run scripts train, layers of up to 512 output channels and
inputs (previous map + skip) of up to 1024.

  model = fg_model.get_model(opt)
  step = FgTrainStep(model)                 # parameters become views of one flat bucket
  out = step.run(x, y_gt, d_gt)             # forward, backward, optimizer: {'loss', 'iou_soft', ..., 'learn_rate'}
  step.sync_model()                         # before model.run / model.statistics / model.prestage see the new weights

One step is image_ops.random_transformation on (x, d_gt, y_gt) -> the cnn / dcnn stack, layer by layer, as
ra_layer_train.ConvBNActPool nodes on the batch moments (the conv, BatchNorm, pool and filter-gradient kernels of the full model's
training step; parameter gradients accumulate in the bucket inside the kernels) -> ra_fg_stats_f32 for the value of the loss
and its pieces -> FgLoss.backward = ra_fg_loss_bwd_f32 -> Adam (epsilon 1e-7, no gradient clip: fg_model.py:260-261) or
momentum 0.9 (:262-263) on the bucket.  The weight-decay terms wd * l2_loss(w) of nnlib.weight_variable belong to total_loss
(:249-250) and reach the update as wd * w inside the optimizer kernels; the fetched 'loss' is without them, as model['loss'].

The stack does not go through the nnlib.cnn / nnlib.dcnn closures: fg_model.get_model builds them for eval, and they hold
the weight tensors they were created with.  sync_model() copies the bucket's values into those tensors.

The wide path is OPT-IN, and the flag is not a tuning knob: the suite pins the default trainer's refusals of wide nets
(tests/test_fg_train.py), so without `wide=True` every check answers as it did before the wide kernels existed.  With it a layer
of more than 128 output channels, or of more than 128 input channels, runs as a WideConvBNActPool node: K1-wide forward
(ra_conv3x3_wide_f32, previous map and skip as two sources, no concat), ra_bn_wide_* BatchNorm, the output-stationary filter
gradient ra_conv3x3_wgrad_wide_acc_f32, and a data gradient per source (ra_layer_train.conv_dgrad on that source's rows of the
filter: K1-wide on a device pack of that output-channel range, ra_conv_wide_pack_weights_dev).  Both nodes live in
ra_layer_train.  The wide path is float32 and uncaptured, and has been measured on synthetic data only.

Not built, refused by name in the constructor: without wide=True, a layer of more than 128 output channels or a dcnn layer
whose input (previous map + skip) has more than 128 channels; with it, a wide layer with a filter size other than 3, more than
128 output channels that are no multiple of 16 or exceed 512, a source of a wide layer that is no multiple of 4 channels, a
source of more than 128 channels that K1-wide cannot produce as a data gradient (no multiple of 16, or more than 512),
compute_dtype = 'bf16'; always: dcnn filter sizes other than 3, the step as one captured HIP graph, several ranks.  Stride-2
wide layers run the full-resolution conv of the zero-stuffed map and ra_subsample_odd_f32, as the narrow ones do: the
sub-pixel form is not built.
"""
import ctypes as C
import math
import os

import numpy as np
import torch

import image_ops
import nnlib as nn
import ra_native as rn
import ra_ops as ops
import ra_train as rt
from ra_layer_train import ConvBNActPool, WideConvBNActPool, _pad_channels, _source_maps, concat_skip, pad4  # noqa: F401
from ra_native import check, ptr

BETA1, BETA2, ADAM_EPS = 0.9, 0.999, 1e-7  # tf.train.AdamOptimizer(learn_rate, epsilon=1e-7), fg_model.py:258-261
MOMENTUM = 0.9                             # tf.train.MomentumOptimizer(learn_rate, momentum=0.9), :262-263
NO_CLIP = float(np.finfo(np.float32).max)  # fg_model.py:265 minimises without clip_by_value: a bound min / max leave inert
IOU_EPS = 1e-5                             # modellib.py:171-181
FETCHES = ('loss', 'foreground_loss', 'iou_soft', 'iou_hard', 'orientation_ce', 'orientation_acc', 'learn_rate')
S = {n: i for i, n in enumerate(ops.FG_STAT_NAMES)}


def loss_pieces(sums, npix, no, segm_loss_fn):
  """The fetches of fg_model.py:208-248 from the nine sums of ra_fg_stats_f32, as float64 scalars on the sums' device.  With
  orientation classes and no foreground pixel orientation_ce, orientation_acc and loss are NaN, the reference's 0 / 0."""
  f_iou_all = lambda inter, a, b: inter / (a + b - inter + IOU_EPS)
  out = {'iou_soft': f_iou_all(sums[S['inter_soft']], sums[S['sum_soft']], sums[S['sum_gt']]),
         'iou_hard': f_iou_all(sums[S['inter_hard']], sums[S['sum_hard']], sums[S['sum_gt']])}
  out['foreground_loss'] = -out['iou_soft'] if segm_loss_fn == 'iou' else sums[S['seg_ce']] / float(npix)
  out['loss'] = out['foreground_loss']
  if no:
    out['orientation_ce'] = sums[S['ori_ce']] / sums[S['mask']]
    out['orientation_acc'] = sums[S['ori_correct']] / sums[S['mask']]
    out['loss'] = out['foreground_loss'] + out['orientation_ce']
  return out


class FgLoss(torch.autograd.Function):
  """The loss head of fg_model.py:196-248 on the logits [B,H,W,nsc + no].  forward: ra_fg_stats_f32 and a few scalar
  operations on its nine sums; backward: ra_fg_loss_bwd_f32, which reads the sums where the forward left them.  meta: nsc, no,
  segm_loss_fn, status (int32 device word the backward writes), pieces (a dict the forward fills with the fetches), upstream
  (a host float used as dL/dloss without looking at the incoming gradient: 1 in the trainer; None: multiply by it)."""

  @staticmethod
  def forward(ctx, logits, y_gt, d_gt, meta):
    logits = logits.contiguous()
    nsc, no = meta['nsc'], meta['no']
    sums = ops.fg_stat_sums(logits, y_gt, d_gt, nsc, no)
    pieces = loss_pieces(sums, logits.numel() // (nsc + no), no, meta['segm_loss_fn'])
    if meta.get('pieces') is not None:
      meta['pieces'].update(pieces)
    ctx.meta, ctx.sums = meta, sums
    ctx.save_for_backward(logits, y_gt, d_gt)
    return pieces['loss'].clone()

  @staticmethod
  def backward(ctx, g):
    logits, y_gt, d_gt = ctx.saved_tensors
    meta = ctx.meta
    up = meta.get('upstream')
    dz, _ = ops.fg_loss_backward(logits, y_gt, d_gt, meta['nsc'], meta['no'], meta['segm_loss_fn'], ctx.sums,
                                 upstream=1.0 if up is None else up, status=meta.get('status'))
    if up is None:
      dz = dz * g.to(dz.dtype)
    return dz, None, None, None


def _layers(d):
  """(scope, index, input channels of the filter, output channels, has BatchNorm) of every layer of the stack."""
  out = []
  for i in range(len(d['cnn_filter_size'])):
    out.append(('cnn', i, d['cnn_channels'][i], d['cnn_channels'][i + 1], d['use_bn']))
  nd = len(d['dcnn_filter_size'])
  for i in range(nd):
    out.append(('dcnn', i, d['dcnn_in_ch'][i], d['dcnn_channels'][i + 1], d['use_bn'] and i < nd - 1))
  return out


WIDE_HINT = '; FgTrainStep(model, wide=True) / fg_model_train.py --train_wide takes the opt-in wide path'


def check_options(opt, d, wide=False):
  """The constructor's refusals that need no device and no library: raised before anything else happens."""
  over = [c for c in d['cnn_channels'][1:] + d['dcnn_channels'][1:] if c > nn.WIDE_COUT]
  if over and not wide:
    raise rn.RecAttendError('fg_model: training with layers of %s output channels is not built (up to %d; eval decodes 3x3 '
                            'layers of up to 512)%s' % (over, nn.WIDE_COUT, WIDE_HINT))
  if wide and opt.get('compute_dtype', 'float32') == 'bf16':
    raise rn.RecAttendError("fg_model: the wide training path is float32; compute_dtype = 'bf16' is not built for it")
  if any(f != 3 for f in d['dcnn_filter_size']):
    raise rn.RecAttendError('fg_model: training with dcnn_filter_size %s is not built (3x3 only; eval decodes any of %s)' %
                            (list(d['dcnn_filter_size']), ops.FILTER_SIZES))
  if opt.get('segm_loss_fn', 'iou') not in ('iou', 'bce'):
    raise rn.RecAttendError('fg_model: segm_loss_fn %r (iou | bce)' % (opt.get('segm_loss_fn'),))
  if opt.get('optimizer', 'adam') not in ('adam', 'momentum'):
    raise rn.RecAttendError('fg_model: optimizer %r (adam | momentum)' % (opt.get('optimizer'),))
  if d['add_orientation']:  # fg_model.py:89-92
    for flag in ('rnd_hflip', 'rnd_vflip', 'rnd_transpose'):
      if opt.get(flag, False):
        raise rn.RecAttendError('fg_model: orientation mode, %s not supported' % flag)
  if any(p not in (1, 2) for p in d['cnn_pool'] + d['dcnn_pool']):
    raise rn.RecAttendError('fg_model: training is built for pool / unpool ratios 1 and 2, got cnn_pool %s, dcnn_pool %s' %
                            (d['cnn_pool'], d['dcnn_pool']))
  world = int(os.environ.get('WORLD_SIZE', '1') or 1)
  if world > 1:
    raise rn.RecAttendError('fg_model: the trainer runs in a single process; WORLD_SIZE = %d (data-parallel fg training is '
                            'not built)' % world)


def _layer_sources(d, scope, i):
  """Channels of the layer's sources: [previous map] or [previous map, skip map]."""
  if scope == 'cnn':
    return [d['cnn_channels'][i]]
  sk = d['dcnn_skip_ch'][i] if d['dcnn_skip_ch'] else 0
  return [d['dcnn_channels'][i]] + ([sk] if sk else [])


def _runs_wide(cin_w, cout):
  """With wide=True a layer runs as a WideConvBNActPool node when its output or its input is beyond K1's 128 channels."""
  return cout > nn.WIDE_COUT or cin_w > nn.WIDE_COUT


def _check_wide_layer(lib, d, scope, i, cin_w, cout, what):
  """check_kernel_forms for a layer that runs as a WideConvBNActPool node: the new plan / support queries instead of a refusal."""
  sources = _layer_sources(d, scope, i)
  ups = int(scope == 'dcnn' and d['dcnn_pool'][i] == 2)
  fs = d['%s_filter_size' % scope][i]
  if fs != 3:
    raise rn.RecAttendError('%s: filter size %d: layers of more than %d input or output channels are trained with 3x3 filters only' %
                            (what, fs, nn.WIDE_COUT))
  cx = sum(pad4(c) for c in sources)
  if cout > nn.WIDE_COUT:
    if cout % 16 or cout > 512:
      raise rn.RecAttendError('%s: a layer of more than %d output channels needs a multiple of 16, up to 512' % (what, nn.WIDE_COUT))
    if any(c % 4 for c in sources):
      raise rn.RecAttendError('%s: the sources of a wide layer (%s channels) must be multiples of 4' % (what, sources))
    if not lib.ra_conv_wide_supported(cx, cout):
      raise rn.RecAttendError('%s: the wide conv takes inputs of up to 1024 channels, got %d' % (what, cx))
    rec = (C.c_int * rn.RA_WGW_PLAN_INTS)()
    for c in sources:
      if lib.ra_conv3x3_wgrad_wide_plan(c, cout, 1, 16, 16, ups, rec) != 0:
        raise rn.RecAttendError('%s: the wide filter gradient refuses the shape: %s' % (what, (lib.ra_last_error_string() or b'').decode()))
  else:  # a narrow layer behind a wide input: K1 and the narrow filter gradient, as without the flag
    if not lib.ra_conv_cout_padded(cout) or not lib.ra_conv_packed_floats(cx, cout):
      raise rn.RecAttendError('%s: no conv / filter-gradient kernel form for these channel counts' % what)
    rec = (C.c_int * rn.RA_PLAN_INTS)()
    if lib.ra_conv3x3_plan(cx, 0, 1, 16, 16, ups, 3, cout, 1, 0, 0, 0, 0, rec) == rn.RA_E_SHAPE:
      raise rn.RecAttendError('%s: the forward conv refuses the shape: %s' % (what, (lib.ra_last_error_string() or b'').decode()))
  if not (scope == 'cnn' and i == 0):  # the data gradient: one conv per source, of that source's channels
    for c in sources:
      ok = lib.ra_conv_wide_supported(pad4(cout), c) if c > nn.WIDE_COUT else lib.ra_conv_packed_floats(pad4(cout), c)
      if not ok:
        raise rn.RecAttendError('%s: the data gradient towards a source of %d channels is a conv of that many output channels: '
                                'beyond %d they must be a multiple of 16, up to 512' % (what, c, nn.WIDE_COUT))


def check_kernel_forms(d, wide=False):
  """Every layer's channel counts against the kernels' own host-side argument checks (forward conv, data gradient, filter
  gradient, BatchNorm), on a nominal 16 x 16 map: a count a kernel form refuses is named here, not in the middle of a step.
  wide: the opt-in wide path (the module docstring says why it is a flag) admits up to 512 output and 1024 input channels."""
  lib = rn.lib()
  rec = (C.c_int * rn.RA_PLAN_INTS)()
  for scope, i, cin_w, cout, bn in _layers(d):
    what = 'fg_model: %s layer %d (%d -> %d channels)' % (scope, i, cin_w, cout)
    if wide and _runs_wide(cin_w, cout):
      _check_wide_layer(lib, d, scope, i, cin_w, cout, what)
      if cout <= nn.WIDE_COUT:  # a narrow layer behind a wide input keeps the narrow BatchNorm kernels; ra_bn_wide_* take any wide count
        _check_bn_forms(lib, d, scope, i, cout, what)
      continue
    cx = pad4(cin_w) if scope == 'cnn' else _dcnn_packed_width(d, i)
    ups = int(scope == 'dcnn' and d['dcnn_pool'][i] == 2)
    mom = int(bn and cout % 4 == 0)
    if not lib.ra_conv_cout_padded(cout) or not lib.ra_conv_packed_floats(cx, cout):
      raise rn.RecAttendError('%s: no conv / filter-gradient kernel form for these channel counts' % what)
    if lib.ra_conv3x3_plan(cx, 0, 1, 16, 16, ups, 3, cout, 1, 0, 0, mom, 0, rec) == rn.RA_E_SHAPE:
      raise rn.RecAttendError('%s: the forward conv refuses the shape: %s' % (what, (lib.ra_last_error_string() or b'').decode()))
    if not (scope == 'cnn' and i == 0):
      if not lib.ra_conv_packed_floats(pad4(cout), cin_w) or \
          lib.ra_conv3x3_plan(pad4(cout), 0, 1, 16, 16, 0, 3, cin_w, 1, 0, 0, 0, 0, rec) == rn.RA_E_SHAPE:
        raise rn.RecAttendError('%s: training a layer whose input — the previous map plus its skip — has %d channels is not '
                                'built: its data gradient is a conv of that many output channels (up to %d)%s' %
                                (what, cin_w, nn.WIDE_COUT, WIDE_HINT))
    _check_bn_forms(lib, d, scope, i, cout, what)


def _check_bn_forms(lib, d, scope, i, cout, what):
  pool = d['cnn_pool'][i] if scope == 'cnn' else 1
  for ps in (rn.RA_BN_PASS_MOMENTS, rn.RA_BN_PASS_FORWARD, rn.RA_BN_PASS_BACKWARD):
    if lib.ra_bn_form(ps, cout, 1, 16, 16, pool, 0, 3, 0) < 0:
      raise rn.RecAttendError('%s: no BatchNorm kernel form for %d channels' % (what, cout))


def _dcnn_packed_width(d, i):
  """Channels of dcnn layer i's kernel input: the previous map and the skip map, each padded to a multiple of 4."""
  sk = d['dcnn_skip_ch'][i] if d['dcnn_skip_ch'] else 0
  return pad4(d['dcnn_channels'][i]) + (pad4(sk) if sk else 0)


class FgTrainStep(object):
  """model.run(['loss', 'train_step'], feed{x, y_gt, d_gt, phase_train=True}) of the reference's fg trainer
  (fg_model_train.py:101-108)."""

  def __init__(self, model, wide=False):
    """wide: the opt-in path for layers of more than 128 output or input channels (the module docstring)."""
    self.model, self.opt, self.d = model, model.opt, model.dims
    self.wide = bool(wide)
    d = self.d
    check_options(self.opt, d, wide=self.wide)
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
      raise rn.RecAttendError('fg_model: the trainer runs in a single process; WORLD_SIZE = %d (data-parallel fg training is '
                              'not built)' % dist.get_world_size())
    check_kernel_forms(d, wide=self.wide)
    if not torch.cuda.is_available():
      raise rn.RecAttendError('fg_model: the training step needs an MI355X (HIP device); there is no CPU fallback')
    self.nsc, self.no = d['nsc'], d['no']
    self.segm_loss_fn = self.opt.get('segm_loss_fn', 'iou')
    self.optimizer = self.opt.get('optimizer', 'adam')
    import fg_model
    names = fg_model.save_var_names(model)  # checkpoint name -> model key
    keys = sorted(names.values())
    dev = torch.device('cuda', torch.cuda.current_device())
    for k in keys:
      if not model[k].is_cuda:
        model[k] = model[k].to(dev)
    # the tensors the eval closures (model.cnn / model.dcnn) were built with: sync_model() writes the bucket's values there
    self._eval_tensors = {k: model[k] for k in keys if k.split('_')[1] in ('w', 'b')}
    self.bucket = rt.GradBucket(model, opt=self.opt, device=dev, names=[k for k in keys if rt.trainable(k)])
    self.accum = torch.zeros_like(self.bucket.param)  # the momentum optimizer's slot
    self.leaves = {}
    for k in self.bucket.names:
      leaf = model[k].detach().requires_grad_(True)  # shares the bucket's storage
      leaf.grad = self.bucket.grad_of[k]             # autograd accumulates straight into the bucket
      self.leaves[k] = leaf
    self.status = torch.zeros((1,), dtype=torch.int32, device=dev)
    self._status_host = torch.zeros((1,), dtype=torch.int32).pin_memory()
    self._status_pending = None
    self._pack = {}
    self.aug_gen = torch.Generator().manual_seed(int(self.opt.get('seed', 1234)))  # augmentation draws (CPU)
    self.last_stats = {}

  # ------------------------------------------------------------------ checkpoint
  def state_dict(self):
    """What a restart needs beyond Model.state_dict_numpy(): the Adam slots as ra_train.GradBucket names them, the momentum
    accumulators under momentum/<name>, and global_step."""
    self.flush_status()
    out = self.bucket.state_dict()
    for k in self.bucket.names:
      o, n, shp = self.bucket.offsets[k]
      out['momentum/' + k] = self.accum[o:o + n].view(shp).detach().cpu().numpy()
    return out

  def load_state_dict(self, state, strict=True):
    self.bucket.load_state_dict(state, strict=strict)
    for k in self.bucket.names:
      o, n, shp = self.bucket.offsets[k]
      if 'momentum/' + k in state:
        v = torch.as_tensor(np.asarray(state['momentum/' + k], dtype=np.float32))
        if tuple(v.shape) != tuple(shp):
          raise rn.RecAttendError('optimizer state momentum/%s: shape %r != %r' % (k, tuple(v.shape), tuple(shp)))
        self.accum[o:o + n].copy_(v.reshape(-1))
      elif strict:
        raise rn.RecAttendError('optimizer state lacks momentum/%s' % k)

  def sync_model(self):
    """The eval closures of fg_model.get_model hold the weight tensors they were built with; the bucket's values go there, so
    that model.run / statistics / prestage evaluate the trained weights.  (BatchNorm tensors are looked up in the model.)"""
    with torch.no_grad():
      for k, t in self._eval_tensors.items():
        t.copy_(self.model[k])
      self.bucket.param.mul_(1.0)  # the optimizer kernel wrote behind torch's version counters: the closures' caches key on them
    return self.model

  # ------------------------------------------------------------------ the graph
  def _check_batch(self, x, y_gt, d_gt):
    for name, t in (('x', x), ('y_gt', y_gt), ('d_gt', d_gt)):
      if t is not None and not (isinstance(t, torch.Tensor) and t.is_cuda):
        raise rn.RecAttendError('FgTrainStep: %s must be a device tensor; there is no CPU path' % name)
    self.model._check_input(x)
    B, H, W = (int(v) for v in x.shape[:3])
    nsc, no = self.nsc, self.no
    if tuple(y_gt.shape) not in (((B, H, W), (B, H, W, 1)) if nsc == 1 else ((B, H, W, nsc),)):
      raise rn.RecAttendError('FgTrainStep: y_gt of shape %r for x %r and %d semantic classes' % (tuple(y_gt.shape), tuple(x.shape), nsc))
    if (d_gt is not None) != bool(no) or (no and tuple(d_gt.shape) != (B, H, W, no)):
      raise rn.RecAttendError('FgTrainStep: d_gt must be [%d,%d,%d,%d] for a net with orientation classes and absent otherwise, '
                              'got %r' % (B, H, W, no, None if d_gt is None else tuple(d_gt.shape)))
    f32 = lambda t: t.to(dtype=torch.float32).contiguous()
    return f32(x), f32(y_gt).reshape(B, H, W, nsc), f32(d_gt) if no else None

  def _layer(self, x, scope, i, bn, meta, stats, skip=None):
    """skip: the layer runs as a WideConvBNActPool node on (x, skip), two sources, instead of ConvBNActPool on one packed input."""
    P = self.leaves
    key = '%s_%d_0' % (scope, i)
    g = self.bucket.grad_of
    if bn and torch.is_grad_enabled():  # the layer's parameter gradients accumulate in the bucket inside the kernels
      meta['grads'] = (g['%s_w_%d' % (scope, i)], g['%s_b_%d' % (scope, i)], g[key + '_gamma'], g[key + '_beta'])
    meta['cache'] = self._pack
    params = (P['%s_w_%d' % (scope, i)], P['%s_b_%d' % (scope, i)], P[key + '_gamma'] if bn else None, P[key + '_beta'] if bn else None)
    if 'c0' in meta:
      y, mean, var = WideConvBNActPool.apply(x, skip, *params, meta)
    else:
      y, mean, var = ConvBNActPool.apply(x, *params, meta)
    if bn:
      stats[key] = (mean, var)
    return y

  def logits(self, x, stats):
    """The cnn / dcnn stack in training mode (fg_model.py:113-167 with phase_train = True): x [B,H,W,inp_depth] -> the last
    dcnn layer's output [B,H,W,nsc + no]; stats receives (batch mean, batch var) per BatchNorm layer."""
    d = self.d
    maps, h = [x], x
    for i in range(len(d['cnn_filter_size'])):
      meta = dict(transposed=False, stride=1, pool=d['cnn_pool'][i], relu=True, chan_map=None)
      if self.wide and _runs_wide(d['cnn_channels'][i], d['cnn_channels'][i + 1]):
        meta.update(c0=h.shape[3], c1=0)
      h = self._layer(_pad_channels(h), 'cnn', i, d['use_bn'], meta, stats)
      maps.append(h)
    nd = len(d['dcnn_filter_size'])
    for i in range(nd):
      cmap, src = None, d['skip_src'][i]
      last = i == nd - 1  # no BatchNorm and no activation on the last layer (fg_model.py:130,155)
      if self.wide and _runs_wide(d['dcnn_in_ch'][i], d['dcnn_channels'][i + 1]):  # previous map and skip as two sources
        sk = maps[src] if src is not None else None
        meta = dict(transposed=True, stride=d['dcnn_pool'][i], pool=1, relu=not last, c0=h.shape[3], c1=sk.shape[3] if sk is not None else 0)
        h = self._layer(_pad_channels(h), 'dcnn', i, d['use_bn'] and not last, meta, stats,
                        skip=_pad_channels(sk) if sk is not None else None)
        continue
      if src is not None:  # concat(prev, skip) (nnlib.py:365) as one packed input; chan_map sends each packed channel to its filter row
        h, cmap = concat_skip(h, maps[src])
      meta = dict(transposed=True, stride=d['dcnn_pool'][i], pool=1, relu=not last, chan_map=cmap)
      h = self._layer(_pad_channels(h), 'dcnn', i, d['use_bn'] and not last, meta, stats)
    return h

  def forward_loss(self, x, y_gt, d_gt=None, draws=None, generator=None):
    """-> (loss, pieces, stats): the loss as a differentiable float64 device scalar, the fetches of fg_model.py:208-248 (plus
    x_trans / y_gt_trans / d_gt_trans) and {BN key: (batch mean, batch var)}.  draws: the augmentation's decisions given
    instead of drawn (image_ops.random_transformation)."""
    x, y_gt, d_gt = self._check_batch(x, y_gt, d_gt)
    opt = self.opt
    self._pack.clear()  # the optimizer wrote the weights through raw pointers since the last pass
    res = image_ops.random_transformation(
        x, int(opt.get('padding', 0) or 0), True, rnd_vflip=bool(opt.get('rnd_vflip', False)), rnd_hflip=bool(opt.get('rnd_hflip', False)),
        rnd_transpose=bool(opt.get('rnd_transpose', False)), rnd_colour=bool(opt.get('rnd_colour', False)), d=d_gt, c=y_gt,
        generator=self.aug_gen if generator is None else generator, draws=draws)
    xt, yt, dt = res['x'], res['c'], res.get('d')
    stats, pieces = {}, {}
    lg = self.logits(xt, stats)
    with torch.no_grad():  # shadow = 0.9 shadow + 0.1 batch statistic (nnlib.py:103-110)
      for key, (mean, var) in stats.items():
        nn._ema_update(self.model[key + '_ema_mean'], self.model[key + '_ema_var'], mean, var)
    meta = dict(nsc=self.nsc, no=self.no, segm_loss_fn=self.segm_loss_fn, status=self.status, pieces=pieces, upstream=1.0)
    loss = FgLoss.apply(lg, yt.contiguous(), dt, meta)
    pieces.update(x_trans=xt, y_gt_trans=yt)
    if dt is not None:
      pieces['d_gt_trans'] = dt
    return loss, pieces, stats

  # ------------------------------------------------------------------ the step
  def _optimizer_step(self, lr):
    b = self.bucket
    lib = rn.lib()
    if self.optimizer == 'adam':
      t = b.global_step + 1
      lr_t = lr * math.sqrt(1.0 - BETA2 ** t) / (1.0 - BETA1 ** t)
      check(lib.ra_adam_step_guarded_f32(ptr(b.param), ptr(b.grad), ptr(b.m), ptr(b.v), ptr(b.wd), b.n, C.c_float(lr_t),
                                         C.c_float(BETA1), C.c_float(BETA2), C.c_float(ADAM_EPS), C.c_float(NO_CLIP),
                                         C.c_float(1.0), ptr(self.status), 0, 1, rn.stream_ptr()), 'ra_adam_step_guarded_f32')
    else:
      check(lib.ra_momentum_step_guarded_f32(ptr(b.param), ptr(b.grad), ptr(self.accum), ptr(b.wd), b.n, C.c_float(lr),
                                             C.c_float(MOMENTUM), C.c_float(1.0), ptr(self.status), 1, rn.stream_ptr()),
            'ra_momentum_step_guarded_f32')
    b.global_step += 1
    self.model['global_step'] = float(b.global_step)

  def flush_status(self):
    """Look at the status word of the LAST step now (run() looks one step late, so that no step waits for the host).  A step
    without a foreground pixel in a net with orientation classes was not applied by the guarded optimizer: its number is given
    back and the batch is reported."""
    rec, self._status_pending = self._status_pending, None
    if rec is not None:
      rec.synchronize()
      if int(self._status_host[0]) != 0:
        self.bucket.global_step = max(0, self.bucket.global_step - 1)
        self.model['global_step'] = float(self.bucket.global_step)
        raise rn.RecAttendError('fg_model training step: the batch has no foreground pixel, so orientation_ce is 0 / 0 (the '
                                'reference trains on NaN here); the update was not applied')

  def run(self, x, y_gt, d_gt=None, draws=None, generator=None, fetch=()):
    """One optimisation step.  Returns the reference's fetches as device scalars (learn_rate as a float), plus those of
    x_trans / y_gt_trans / d_gt_trans named in `fetch`."""
    self.flush_status()
    self.bucket.zero_grad()
    loss, pieces, stats = self.forward_loss(x, y_gt, d_gt, draws=draws, generator=generator)
    loss.backward()
    lr = rt.learn_rate(self.opt, self.bucket.global_step)
    self._optimizer_step(lr)
    self._status_host.copy_(self.status, non_blocking=True)
    ev = torch.cuda.Event()
    ev.record()
    self._status_pending = ev
    self.last_stats = stats
    out = {k: pieces[k].detach() for k in FETCHES if k in pieces}
    out['learn_rate'] = lr
    for k in fetch:
      if k not in ('x_trans', 'y_gt_trans', 'd_gt_trans') or k not in pieces:
        raise KeyError(k)
      out[k] = pieces[k]
    return out
