"""Oracle of fg_model's training graph (fg_model.py:94-266 of the reference) in torch on the CPU, float64 by default, for the
option dictionaries of tests/fg_oracle.py: the augmentation with given draws, conv + bias -> BatchNorm on the batch moments ->
ReLU -> max-pool, the transposed convs with their skip inputs, the loss head with its eps inside the logarithms,
wd * l2_loss(w), autograd for every gradient, and one Adam / one momentum update restated in float64.  Written from the
reference's mathematics; the reference itself (TensorFlow 0.12) cannot be run.  `dtype=torch.float32` runs the same graph in
plain float32, to tell a float32 deviation from a wrong kernel.

Weights are addressed by the checkpoint names of get_save_var (fg_model.py:270-285), as in fg_oracle."""
import numpy as np
import torch
import torch.nn.functional as F

import fg_oracle as fo

BN_EPS = 1e-3    # nnlib.py:119
LOG_EPS = 1e-5   # modellib.py:418-427
IOU_EPS = 1e-5   # modellib.py:171-181
EMA_DECAY = 0.9  # nnlib.py:103-104 with phase_train = 1


def augment(opt, x, y_gt, d_gt=None, draws=None):
  """image_ops.random_transformation with phase_train = True and given draws {off_y, off_x}: zero padding of `padding` pixels,
  then the crop of the input's size at the offset (image_ops.py:36-67), on x, c = y_gt and d = d_gt alike.  NumPy arrays,
  channels last.  The nets of this oracle train without flips, transpose and colour jitter (fg_model_train.py:487-490)."""
  pad = int(opt.get('padding', 0) or 0)
  draws = draws or {}
  if any(draws.get(k) for k in ('flip_v', 'flip_h', 'transpose')) or opt.get('rnd_colour'):
    raise NotImplementedError('the oracle restates the crop only')
  oy, ox = int(draws.get('off_y', pad)), int(draws.get('off_x', pad))
  assert 0 <= oy <= 2 * pad and 0 <= ox <= 2 * pad

  def one(a):
    if a is None:
      return None
    a = np.asarray(a)
    H, W = a.shape[1:3]
    width = [(0, 0), (pad, pad), (pad, pad)] + [(0, 0)] * (a.ndim - 3)
    return np.ascontiguousarray(np.pad(a, width)[:, oy:oy + H, ox:ox + W])

  return one(x), one(y_gt), one(d_gt)


def _conv_transpose_same(h, w, s):
  """tf.nn.conv2d_transpose(h, w [f,f,out,in], stride s, SAME) to the size n * s, channels first."""
  f = w.shape[0]
  tot = max(f - s, 0)
  lo = tot // 2
  full = F.conv_transpose2d(h, w.permute(3, 2, 0, 1), None, stride=s)
  Ho, Wo = h.shape[2] * s, h.shape[3] * s
  full = F.pad(full, (0, max(0, lo + Wo - full.shape[3]), 0, max(0, lo + Ho - full.shape[2])))
  return full[:, :, lo:lo + Ho, lo:lo + Wo]


def _bn_train(u, gamma, beta):
  mean = u.mean(dim=(0, 2, 3))
  var = ((u - mean.view(1, -1, 1, 1)) ** 2).mean(dim=(0, 2, 3))  # tf.nn.moments: biased
  y = gamma.view(1, -1, 1, 1) * (u - mean.view(1, -1, 1, 1)) * torch.rsqrt(var.view(1, -1, 1, 1) + BN_EPS) + beta.view(1, -1, 1, 1)
  return y, mean, var


def logits(opt, T, x):
  """The stack with phase_train = True.  T: checkpoint name -> torch tensor; x [B,H,W,D] torch.  Returns (logits [B,H,W,C],
  {layer prefix: (batch mean, batch var)})."""
  cnn_ch, dcnn_ch, src = fo.wiring(opt)
  bn = opt.get('use_bn', True)
  h = x.permute(0, 3, 1, 2)
  maps, moments = [h], {}
  for i in range(len(cnn_ch) - 1):
    pre = 'cnn/layer_%d' % i
    h = F.conv2d(h, T[pre + '/w'].permute(3, 2, 0, 1), T[pre + '/b'], padding=1)
    if bn:
      h, mean, var = _bn_train(h, T[pre + '/bn/gamma'], T[pre + '/bn/beta'])
      moments[pre] = (mean, var)
    h = torch.relu(h)
    if opt['cnn_pool'][i] > 1:
      h = F.max_pool2d(h, opt['cnn_pool'][i], opt['cnn_pool'][i])
    maps.append(h)
  nd = len(dcnn_ch) - 1
  for i in range(nd):
    pre = 'dcnn/layer_%d' % i
    if src[i] is not None:
      h = torch.cat([h, maps[src[i]]], dim=1)
    h = _conv_transpose_same(h, T[pre + '/w'], opt['dcnn_pool'][i]) + T[pre + '/b'].view(1, -1, 1, 1)
    if i < nd - 1:
      if bn:
        h, mean, var = _bn_train(h, T[pre + '/bn/gamma'], T[pre + '/bn/beta'])
        moments[pre] = (mean, var)
      h = torch.relu(h)
  return h.permute(0, 2, 3, 1), moments


def loss_pieces(z, y_gt, d_gt, nsc, no, segm_loss_fn):
  """fg_model.py:196-248 on the logits z [..., nsc + no] (torch, any float dtype; differentiable).  y_gt [..., nsc], d_gt
  [..., 8] or None.  Returns the reference's fetches as 0-d tensors."""
  z = z.reshape(-1, nsc + no)
  g = y_gt.reshape(-1, nsc).to(z.dtype)
  npix = z.shape[0]
  f_iou_all = lambda a, b: (a * b).sum() / (a.sum() + b.sum() - (a * b).sum() + IOU_EPS)
  if nsc == 1:
    p = torch.sigmoid(z[:, :1])
    hard = (z[:, :1] > 0).to(z.dtype)
    mask = g
    iou_soft, iou_hard = f_iou_all(p, g), f_iou_all(hard, g)
    seg = (-g * torch.log(p + LOG_EPS) - (1 - g) * torch.log(1 - p + LOG_EPS)).sum() / npix  # f_bce
  else:
    zs = z[:, :nsc]
    p = torch.softmax(zs, dim=1)
    hard = (zs == zs.max(dim=1, keepdim=True).values).to(z.dtype)  # y_out == max(y_out), on the logits
    mask = g[:, 1:].max(dim=1, keepdim=True).values
    iou_soft, iou_hard = f_iou_all(p[:, 1:], g[:, 1:]), f_iou_all(hard[:, 1:], g[:, 1:])
    seg = (-g * torch.log(p + LOG_EPS)).sum() / npix  # f_ce over all channels
  out = {'iou_soft': iou_soft, 'iou_hard': iou_hard}
  out['foreground_loss'] = -iou_soft if segm_loss_fn == 'iou' else seg
  out['loss'] = out['foreground_loss']
  if no:
    t = d_gt.reshape(-1, no).to(z.dtype)
    d = torch.softmax(z[:, nsc:], dim=1)
    ce = (-t * torch.log(d + LOG_EPS)).sum(dim=1, keepdim=True)
    out['orientation_ce'] = (ce * mask).sum() / mask.sum()
    correct = (z[:, nsc:].argmax(dim=1) == t.argmax(dim=1)).to(z.dtype).unsqueeze(1)
    out['orientation_acc'] = (correct * mask).sum() / mask.sum()
    out['loss'] = out['foreground_loss'] + out['orientation_ce']
  return out


def loss_grad(z, y_gt, d_gt, nsc, no, segm_loss_fn):
  """dloss / dz by float64 autograd of loss_pieces.  NumPy in, NumPy float64 out, z's shape."""
  zt = torch.from_numpy(np.asarray(z, np.float64)).clone().requires_grad_(True)
  t = lambda a: None if a is None else torch.from_numpy(np.asarray(a, np.float64))
  loss_pieces(zt, t(y_gt), t(d_gt), nsc, no, segm_loss_fn)['loss'].backward()
  return zt.grad.numpy()


def loss_grad_formulas(z, y_gt, d_gt, nsc, no, segm_loss_fn, dtype=torch.float32):
  """The closed forms the device kernel evaluates, in `dtype` torch on the CPU: p by 1 / (1 + exp(-z)) or exp(z - max) / sum,
  the batch-wide terms 1 / U, I / U^2 and 1 / MASK formed in float64 from float64 sums and rounded once, then
    bce  q = (-g / (p + eps) + (1 - g) / (1 - p + eps)) / npix        |  q_c = -g_c / (p_c + eps) / npix
    iou  q = -(g / U - (I / U^2)(1 - g)), over c >= 1 for nsc > 1
    dz = q p (1 - p)                                                  |  dz_c = p_c (q_c - sum_j p_j q_j)
    orientation: q_k = -t_k m / (d_k + eps) / MASK, the same softmax adjoint.
  NumPy in, NumPy float64 out."""
  z64 = torch.from_numpy(np.asarray(z, np.float64)).reshape(-1, nsc + no)
  g64 = torch.from_numpy(np.asarray(y_gt, np.float64)).reshape(-1, nsc)
  npix = z64.shape[0]
  if nsc == 1:
    p64, gf = torch.sigmoid(z64[:, :1]), g64
    m64 = g64
  else:
    p64, gf = torch.softmax(z64[:, :nsc], dim=1)[:, 1:], g64[:, 1:]
    m64 = g64[:, 1:].max(dim=1, keepdim=True).values
  I = float((p64 * gf).sum())
  U = float(p64.sum()) + float(gf.sum()) - I + IOU_EPS
  c = lambda v: torch.tensor(v, dtype=torch.float64).to(dtype)
  inv_u, i_u2, inv_n = c(1.0 / U), c(I / (U * U)), c(1.0 / npix)
  zz, g = z64.to(dtype), g64.to(dtype)
  eps = torch.tensor(LOG_EPS, dtype=dtype)
  if nsc == 1:
    p = 1 / (1 + torch.exp(-zz[:, :1]))
    q = (-g / (p + eps) + (1 - g) / (1 - p + eps)) * inv_n if segm_loss_fn == 'bce' else -(g * inv_u - i_u2 * (1 - g))
    dz = [q * (p * (1 - p))]
  else:
    zs = zz[:, :nsc]
    e = torch.exp(zs - zs.max(dim=1, keepdim=True).values)
    p = e / e.sum(dim=1, keepdim=True)
    if segm_loss_fn == 'bce':
      q = -g / (p + eps) * inv_n
    else:
      q = -(g * inv_u - i_u2 * (1 - g))
      q[:, 0] = 0
    dz = [p * (q - (p * q).sum(dim=1, keepdim=True))]
  if no:
    t = torch.from_numpy(np.asarray(d_gt, np.float64)).reshape(-1, no).to(dtype)
    mask = float(m64.sum())
    zo = zz[:, nsc:]
    e = torch.exp(zo - zo.max(dim=1, keepdim=True).values)
    d = e / e.sum(dim=1, keepdim=True)
    if mask > 0:
      q = -t * m64.to(dtype) / (d + eps) * c(1.0 / mask)
      dz.append(d * (q - (d * q).sum(dim=1, keepdim=True)))
    else:
      dz.append(torch.zeros_like(d))
  return torch.cat(dz, dim=1).to(torch.float64).numpy().reshape(np.asarray(z).shape)


def train_graph(opt, P, x, y_gt, d_gt=None, draws=None, dtype=torch.float64):
  """One forward / backward pass of the training graph on the batch.  P: checkpoint name -> array (fo.random_weights).
  Returns {'pieces': {fetch: float}, 'total_loss': float (with wd * l2_loss(w)), 'grads': {name: array} of total_loss (the
  weight-decay term included, as the optimizer sees it), 'data_grads': the same without it, 'moments': {layer: (mean, var)},
  'ema': {name: array} the shadows after this step, 'logits', 'x_trans', 'y_gt_trans', 'd_gt_trans'}."""
  nsc = int(opt.get('num_semantic_classes', 1))
  no = int(opt['num_orientation_classes']) if opt.get('add_orientation') else 0
  seg = opt.get('segm_loss_fn', 'iou')
  wd = float(opt.get('weight_decay', 0.0) or 0.0)
  xt, yt, dt = augment(opt, x, np.asarray(y_gt).reshape(np.asarray(x).shape[:3] + (nsc,)), d_gt if no else None, draws)
  t = lambda a: None if a is None else torch.from_numpy(np.asarray(a, np.float64)).to(dtype)
  T = {k: t(v).clone().requires_grad_(not k.endswith(('ema_mean', 'ema_var'))) for k, v in P.items()}
  z, moments = logits(opt, T, t(xt))
  pieces = loss_pieces(z, t(yt), t(dt), nsc, no, seg)
  train = [k for k in sorted(T) if T[k].requires_grad]
  data_grads = torch.autograd.grad(pieces['loss'], [T[k] for k in train], allow_unused=True)
  grads, total = {}, pieces['loss'].detach().clone()
  for k, gk in zip(train, data_grads):
    gk = torch.zeros_like(T[k]) if gk is None else gk
    if wd and k.endswith('/w'):  # nnlib.weight_variable: wd * tf.nn.l2_loss(w) = wd * sum(w^2) / 2, filters only
      total = total + wd * (T[k].detach() ** 2).sum() / 2
      grads[k] = (gk + wd * T[k].detach()).to(torch.float64).numpy()
    else:
      grads[k] = gk.to(torch.float64).numpy()
  ema = {}
  for pre, (mean, var) in moments.items():
    ema[pre + '/bn/ema_mean'] = (EMA_DECAY * T[pre + '/bn/ema_mean'] + (1 - EMA_DECAY) * mean.detach()).to(torch.float64).numpy()
    ema[pre + '/bn/ema_var'] = (EMA_DECAY * T[pre + '/bn/ema_var'] + (1 - EMA_DECAY) * var.detach()).to(torch.float64).numpy()
  f8 = lambda a: a.detach().to(torch.float64).numpy()
  return dict(pieces={k: float(v.detach()) for k, v in pieces.items()}, total_loss=float(total), grads=grads,
              data_grads={k: (np.zeros(tuple(T[k].shape)) if gk is None else f8(gk)) for k, gk in zip(train, data_grads)},
              moments={k: (f8(m), f8(v)) for k, (m, v) in moments.items()}, ema=ema, logits=f8(z), x_trans=xt, y_gt_trans=yt,
              d_gt_trans=dt)


def learn_rate(opt, step):
  """tf.train.exponential_decay(base, step, steps_per_decay, decay, staircase=True), fg_model.py:252-257."""
  return float(opt.get('base_learn_rate', 1e-3)) * float(opt.get('learn_rate_decay', 0.96)) ** (
      int(step) // int(opt.get('steps_per_learn_rate_decay', 5000)))


def adam_step(p, g, m, v, lr, t, beta1=0.9, beta2=0.999, eps=1e-7):
  """tf.train.AdamOptimizer(lr, epsilon=eps) at its t-th application, float64 arrays: (p, m, v) afterwards."""
  p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
  lr_t = lr * np.sqrt(1 - beta2 ** t) / (1 - beta1 ** t)
  m = beta1 * m + (1 - beta1) * g
  v = beta2 * v + (1 - beta2) * g * g
  return p - lr_t * m / (np.sqrt(v) + eps), m, v


def momentum_step(p, g, accum, lr, momentum=0.9):
  """tf.train.MomentumOptimizer(lr, momentum), float64 arrays: (p, accum) afterwards."""
  p, g, accum = (np.asarray(a, np.float64) for a in (p, g, accum))
  accum = momentum * accum + g
  return p - lr * accum, accum
