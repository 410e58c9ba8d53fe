"""fg_model at eval: the fully convolutional pre-stage that produces y_in (foreground / semantic classes) and d_in (eight
orientation classes) for full_model and box_model (fg_model.py:11-267 of the reference; its outputs reach the decode loop
through fg_model_pack.py and the dataset reader as 8-bit images).

`get_model(opt)` takes the reference's option dictionary (fg_model.py:14-68, fg_model_train.py:451-500) and returns a
`Model`: the reference's `model` dict (`model['cnn_w_0']`, `model['dcnn_3_0_gamma']`, ...) with `run()`, strict
`load_weights()` under the checkpoint names of get_save_var (fg_model.py:270-285) and `prestage()`.  The net is nnlib.cnn
followed by nnlib.dcnn with skip connections; layers of up to 128 output channels run K1, wider ones the wide kernel
(ra_ops.conv_wide), the head is one kernel (ra_ops.fg_head).  Eval only: `phase_train = True` and the outputs of the loss
raise RecAttendError.  `Model.statistics(x, y_gt, d_gt)` gives the numbers the reference's Evaluator logs (the IoUs, the losses,
the orientation accuracy) from one pass over the logits (ra_ops.fg_statistics); fg_model_eval.py is the command line.
"""
import numpy as np
import torch

import nnlib as nn
import ra_ops as ops
from ra_native import RecAttendError

BN_NAMES = ('beta', 'gamma', 'ema_mean', 'ema_var')


def derive(opt):
  """The net's static description from the option dictionary (fg_model.py:14-68, :112-177)."""
  d = {}
  d['inp_depth'] = opt['inp_depth']
  cnn_depth = list(opt['cnn_depth'])
  ncnn = len(cnn_depth)
  d['cnn_filter_size'] = [3] * ncnn  # whatever the option says (fg_model.py:114)
  d['cnn_channels'] = [d['inp_depth']] + cnn_depth
  d['cnn_pool'] = list(opt['cnn_pool'])
  d['dcnn_filter_size'] = list(opt['dcnn_filter_size']) if 'dcnn_filter_size' in opt else [3] * len(opt['dcnn_depth'])
  ndcnn = len(d['dcnn_filter_size'])
  d['dcnn_channels'] = [d['cnn_channels'][-1]] + list(opt['dcnn_depth'])
  d['dcnn_pool'] = list(opt['dcnn_pool'])
  d['use_bn'] = bool(opt.get('use_bn', True))
  add_skip = bool(opt.get('add_skip_conn', False))
  if 'cnn_skip_mask' in opt:
    cnn_skip_mask = list(opt['cnn_skip_mask'])
  elif 'cnn_skip' in opt:
    cnn_skip_mask = list(opt['cnn_skip'])
  else:
    cnn_skip_mask = [add_skip] * ncnn
  dcnn_skip_mask = list(opt['dcnn_skip_mask']) if 'dcnn_skip_mask' in opt else cnn_skip_mask[::-1]
  d['add_orientation'] = bool(opt.get('add_orientation', False))
  d['no'] = int(opt['num_orientation_classes']) if d['add_orientation'] else 0
  d['nsc'] = int(opt.get('num_semantic_classes', 1))
  if len(d['cnn_pool']) != ncnn or len(d['dcnn_channels']) != ndcnn + 1 or len(d['dcnn_pool']) != ndcnn:
    raise RecAttendError('fg_model: cnn_depth / cnn_pool and dcnn_filter_size / dcnn_depth / dcnn_pool lists differ in length')
  # skip wiring (fg_model.py:131-153): the mask runs over [x] + h_cnn[:-1]; the selected maps are consumed from the deepest
  # upwards by the dcnn mask's entries; the first dcnn layer never has one.  skip_src[i]: index into [x] + h_cnn, or None
  if add_skip:
    picked = [k for k, sk in zip(range(ncnn), cnn_skip_mask) if sk]
    skip_src, counter = [None], len(picked) - 1
    for sk in dcnn_skip_mask:
      if sk:
        if counter < 0:
          raise RecAttendError('fg_model: dcnn_skip_mask asks for more skip connections than cnn_skip_mask selects')
        skip_src.append(picked[counter])
        counter -= 1
      else:
        skip_src.append(None)
    skip_src = (skip_src + [None] * ndcnn)[:ndcnn]
    d['skip_src'] = skip_src
    d['dcnn_skip_ch'] = [0 if k is None else d['cnn_channels'][k] for k in skip_src]
  else:
    skip_src = d['skip_src'] = [None] * ndcnn
    d['dcnn_skip_ch'] = None
  want = d['nsc'] + d['no']
  if d['dcnn_channels'][-1] != want:  # fg_model.py:168-177
    raise RecAttendError('fg_model: expecting the last dcnn channel count to be %d (%d semantic + %d orientation classes), got %d' %
                         (want, d['nsc'], d['no'], d['dcnn_channels'][-1]))
  if not 1 <= d['nsc'] <= 16 or d['no'] not in (0, 8):
    raise RecAttendError('fg_model: the head is built for 1 .. 16 semantic and 0 or 8 orientation classes')
  d['pool_total'] = int(np.prod(d['cnn_pool']))
  # map size (as a fraction of the input) of [x] + h_cnn and of every dcnn layer's input: a skip must meet a map of its own size
  down = [1]
  for p in d['cnn_pool']:
    down.append(down[-1] * p)
  cur = down[-1]
  for i in range(ndcnn):
    if skip_src[i] is not None and down[skip_src[i]] != cur:
      raise RecAttendError('fg_model: dcnn layer %d reads a map at 1/%d of the input but its skip source is at 1/%d' %
                           (i, cur, down[skip_src[i]]))
    if cur % d['dcnn_pool'][i]:
      raise RecAttendError('fg_model: dcnn_pool upsamples past the input size at layer %d' % i)
    cur //= d['dcnn_pool'][i]
  if cur != 1:
    raise RecAttendError('fg_model: the dcnn ends at 1/%d of the input size' % cur)
  d['dcnn_in_ch'] = [d['dcnn_channels'][i] + (d['dcnn_skip_ch'][i] if d['dcnn_skip_ch'] else 0) for i in range(ndcnn)]
  return d


def save_var_names(model):
  """Checkpoint name -> model key, as get_save_var (fg_model.py:270-285) without its `step`."""
  out = {}
  for net in ('cnn', 'dcnn'):
    ii = 0
    while '{}_w_{}'.format(net, ii) in model:
      for w in ('w', 'b'):
        out['{}/layer_{}/{}'.format(net, ii, w)] = '{}_{}_{}'.format(net, w, ii)
      for w in BN_NAMES:
        key = '{}_{}_{}_{}'.format(net, ii, 0, w)
        if key in model:
          out['{}/layer_{}/bn/{}'.format(net, ii, w)] = key
      ii += 1
  return out


class Model(dict):
  """The reference's `model` dict of fg_model plus run() / prestage().  Tensor-valued entries are weights."""

  OUTPUTS = ('y_out', 'd_out')
  TRAIN_ONLY = ('loss', 'foreground_loss', 'iou_soft', 'iou_hard', 'orientation_ce', 'orientation_acc', 'train_step',
                'x_trans', 'y_gt_trans', 'd_gt_trans')

  def __init__(self, opt, d):
    dict.__init__(self)
    self.opt = dict(opt)
    self.dims = d
    self.cnn = self.dcnn = None

  def weight_keys(self):
    return sorted(save_var_names(self))

  def load_weights(self, weights, strict=True):
    """weights: mapping checkpoint name (cnn/layer_i/{w,b}, cnn/layer_i/bn/{beta,gamma,ema_mean,ema_var}, same for dcnn) ->
    array.  strict (default): every registered tensor must be present.  `step` is accepted and ignored."""
    names = save_var_names(self)
    given = set(k for k in weights.keys() if k != 'step')
    if strict:
      missing = sorted(set(names) - given)
      if missing:
        raise RecAttendError('load_weights: %d registered tensors are missing from the archive (first: %s)' %
                             (len(missing), ', '.join(missing[:4])))
    extra = sorted(given - set(names))
    if extra:
      import warnings
      warnings.warn('load_weights: ignoring %d unknown keys (first: %s)' % (len(extra), ', '.join(extra[:4])))
    for k in sorted(given & set(names)):
      v = torch.as_tensor(np.asarray(weights[k], dtype=np.float32))
      t = self[names[k]]
      if tuple(v.shape) != tuple(t.shape):
        raise RecAttendError('weight %s: shape %r != %r' % (k, tuple(v.shape), tuple(t.shape)))
      t.copy_(v)
    return self

  def state_dict_numpy(self):
    names = save_var_names(self)
    return {k: self[names[k]].detach().cpu().numpy() for k in sorted(names)}

  # ------------------------------------------------------------------ forward
  def _check_input(self, x):
    d = self.dims
    if len(x.shape) != 4 or x.shape[3] != d['inp_depth']:
      raise RecAttendError('fg_model: x of shape %r, expected [B,H,W,%d]' % (tuple(x.shape), d['inp_depth']))
    p = d['pool_total']
    if x.shape[1] % p or x.shape[2] % p:
      raise RecAttendError('fg_model: input height and width must be multiples of the net\'s total pooling factor %d, got %d x %d' %
                           (p, x.shape[1], x.shape[2]))

  def logits(self, x):
    """x [B,H,W,inp_depth] (device tensor) -> the last dcnn layer's output [B,H,W,nsc + no] (fg_model.py:112-160)."""
    d = self.dims
    h_cnn = self.cnn(x, copy_idx=0)
    maps = [x] + h_cnn
    skip = [None if k is None else maps[k] for k in d['skip_src']]
    h_dcnn = self.dcnn(h_cnn[-1], skip=skip if d['dcnn_skip_ch'] else None, copy_idx=0)
    return h_dcnn[-1]

  def _device_input(self, x):
    if not isinstance(x, torch.Tensor):
      x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    self._check_input(x)
    if not torch.cuda.is_available():
      raise RecAttendError('fg_model needs an MI355X (HIP device); no CPU fallback')
    return x.to(device='cuda', dtype=torch.float32).contiguous()

  def prestage(self, x, quantise=True, into=None):
    """(y_in [B,H,W,nsc], d_in [B,H,W,no] or None) as device tensors: y_out / d_out, by default through the 8-bit round trip
    the decode loop sees in the reference (floor(v * 255) / 255: fg_model_pack.py:41-48, ins_seg_dataset.py:273-292).
    into: a DecodeEngine (or a DecodePipeline slot, (engine, stream)) — the head also writes that engine's packed input
    image and d_in / y_in buffers, and the returned tensors are those buffers; decode with
    engine.forward(x, prepacked=True)."""
    d = self.dims
    x = self._device_input(x)
    lg = self.logits(x)
    if into is None:
      return ops.fg_head(lg, d['nsc'], d['no'], quantise=quantise)
    eng = into[0] if isinstance(into, tuple) else into
    ed = eng.d
    if (ed['H'], ed['W'], ed['D']) != tuple(x.shape[1:]) or not d['no'] or not ed.get('add_d_out') or not ed.get('add_y_out') or \
        ed['nsc'] != d['nsc']:
      raise RecAttendError('prestage(into=): the engine decodes %d x %d x %d images with d_in (8) and y_in (%d); this net gives '
                           '%r with %d + %d classes' % (ed['H'], ed['W'], ed['D'], ed['nsc'], tuple(x.shape[1:]), d['nsc'], d['no']))
    B = x.shape[0]
    subs = eng.prestage_slots(B)
    Bs = B // len(subs)
    for k, sb in enumerate(subs):
      sb['x'].copy_(x[k * Bs:(k + 1) * Bs])
      ops.fg_head(lg[k * Bs:(k + 1) * Bs], d['nsc'], d['no'], quantise=quantise, y_out=sb['y_in'], d_out=sb['d_in'], x=sb['x'],
                  packed=sb['img'])
    return eng.glob['y_in'], eng.glob['d_in']

  def statistics(self, x, y_gt, d_gt=None):
    """What the reference's Evaluator logs for this net (fg_model_train.py:131-133; fg_model.py:196-248) on one batch, as a dict
    of Python floats computed in float64 from one pass over the logits (ops.fg_statistics): iou_soft, iou_hard,
    foreground_loss (-iou_soft for segm_loss_fn 'iou', the summed (b)ce / (B H W) for 'bce'), loss, and with orientation
    orientation_ce and orientation_acc (NaN where the ground truth has no foreground pixel, as the reference's 0 / 0).
    x [B,H,W,inp_depth]; y_gt [B,H,W] or [B,H,W,nsc]; d_gt [B,H,W,8] with orientation.  The hard IoU and the accuracy are
    taken on the logits, see ops.fg_statistics.  The outputs of the loss stay refused by run(): nothing here trains."""
    d = self.dims
    nsc, no = d['nsc'], d['no']
    seg = self.opt.get('segm_loss_fn', 'iou')
    if seg not in ('iou', 'bce'):
      raise RecAttendError('fg_model.statistics: segm_loss_fn %r (iou | bce)' % (seg,))
    for name, t in (('x', x), ('y_gt', y_gt), ('d_gt', d_gt)):
      if t is not None and not (isinstance(t, torch.Tensor) and t.is_cuda):
        raise RecAttendError('fg_model.statistics: %s must be a device tensor; there is no CPU path' % name)
    self._check_input(x)
    B, H, W = (int(v) for v in x.shape[:3])
    if tuple(y_gt.shape) not in (((B, H, W), (B, H, W, 1)) if nsc == 1 else ((B, H, W, nsc),)):
      raise RecAttendError('fg_model.statistics: y_gt of shape %r for x %r and %d semantic classes' % (tuple(y_gt.shape), tuple(x.shape), nsc))
    if d_gt is not None and not no:
      raise RecAttendError('fg_model.statistics: d_gt given, but the net was built without add_orientation')
    if no and (d_gt is None or tuple(d_gt.shape) != (B, H, W, no)):
      raise RecAttendError('fg_model.statistics: the net has orientation classes: d_gt must be [%d,%d,%d,%d], got %r' % (
          B, H, W, no, None if d_gt is None else tuple(d_gt.shape)))
    f32 = lambda t: t.to(dtype=torch.float32).contiguous()
    s = ops.fg_statistics(self.logits(f32(x)), f32(y_gt), f32(d_gt) if no else None, nsc, no)
    f_iou_all = lambda inter, a, b: inter / (a + b - inter + 1e-5)  # modellib.py:171-181
    out = {'iou_soft': f_iou_all(s['inter_soft'], s['sum_soft'], s['sum_gt']),
           'iou_hard': f_iou_all(s['inter_hard'], s['sum_hard'], s['sum_gt'])}
    out['foreground_loss'] = -out['iou_soft'] if seg == 'iou' else s['seg_ce'] / float(B * H * W)  # :221-233
    out['loss'] = out['foreground_loss']
    if no:
      nan = float('nan')
      out['orientation_ce'] = s['ori_ce'] / s['mask'] if s['mask'] else (nan if s['ori_ce'] == 0 else s['ori_ce'] * float('inf'))
      out['orientation_acc'] = s['ori_correct'] / s['mask'] if s['mask'] else nan  # :244-245: 0 / 0
      out['loss'] = out['foreground_loss'] + out['orientation_ce']  # :240
    return out

  def run(self, outputs, feed, as_numpy=False):
    single = isinstance(outputs, str)
    names = [outputs] if single else list(outputs)
    for n in names:
      if n in self.TRAIN_ONLY:
        raise RecAttendError('fg_model: output %r needs the loss / the training graph: this build is eval only' % n)
      if n not in self.OUTPUTS:
        raise KeyError(n)
    if nn._is_train(feed.get('phase_train', False)):
      raise RecAttendError('fg_model: phase_train = True: this build is eval only')
    if 'd_out' in names and not self.dims['no']:
      raise KeyError('d_out (the model was built without add_orientation)')
    self._check_input(np.asarray(feed['x']) if not isinstance(feed['x'], torch.Tensor) else feed['x'])
    y, dd = self.prestage(feed['x'], quantise=False)
    res = [y if n == 'y_out' else dd for n in names]
    if as_numpy:
      torch.cuda.synchronize()
      res = [r.detach().cpu().numpy() for r in res]
    return res[0] if single else res


def get_model(opt, device=None):
  """fg_model.py:11-267 at eval.  Option keys: inp_depth, cnn_filter_size (forced to 3), cnn_depth, cnn_pool,
  dcnn_filter_size, dcnn_depth, dcnn_pool, use_bn, add_skip_conn, cnn_skip_mask | cnn_skip, dcnn_skip_mask,
  add_orientation, num_orientation_classes, num_semantic_classes; the training keys are accepted and unused."""
  d = derive(opt)
  model = Model(opt, d)
  ncnn, ndcnn = len(d['cnn_filter_size']), len(d['dcnn_filter_size'])
  model.cnn = nn.cnn(d['cnn_filter_size'], d['cnn_channels'], d['cnn_pool'], [nn.relu] * ncnn, [d['use_bn']] * ncnn,
                     phase_train=False, model=model)
  # the last dcnn layer has no BN and no activation (fg_model.py:130,155)
  model.dcnn = nn.dcnn(d['dcnn_filter_size'], d['dcnn_channels'], d['dcnn_pool'], [nn.relu] * (ndcnn - 1) + [None],
                       [d['use_bn']] * (ndcnn - 1) + [False], skip_ch=d['dcnn_skip_ch'], phase_train=False, model=model)
  model.cnn.declare_copies(1)
  model.dcnn.declare_copies(1)
  return model
