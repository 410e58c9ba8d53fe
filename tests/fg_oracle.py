"""Oracles of fg_model at eval (fg_model.py:112-194 of the reference): a float64 NumPy restatement on oracle/ra_oracle.py's
primitives and, beside it, an independent torch-CPU restatement in channels-first layout (conv_transpose2d), the way
oracle/ra_oracle_torch.py stands beside ra_oracle.py.  The reference itself (TensorFlow 0.12) cannot be run, so the two
pin each other; tests/test_fg_model.py holds them to 1e-9.

Weights are addressed by the checkpoint names of get_save_var (fg_model.py:270-285)."""
import numpy as np

import ra_oracle as ora

BN = ('beta', 'gamma', 'ema_mean', 'ema_var')


def kitti_opt():
  """run_kitti.sh:13-28 through fg_model_train.py:451-500."""
  s = lambda t: [int(v) for v in t.split(',')]
  m = lambda t: [v == '1' for v in t.split(',')]
  cd, dd = s('32,64,64,96,96,128,128,128,128,128,128,128,128,256,256,256,256,512'), s('256,256,128,128,96,96,64,64,32,32,9')
  return dict(inp_depth=3, padding=16, cnn_filter_size=[3] * len(cd), cnn_depth=cd, cnn_pool=s('1,2,1,2,1,2,1,1,1,1,1,1,1,2,1,1,1,2'),
              cnn_skip_mask=m('1,0,0,0,0,1,0,0,0,0,0,0,0,1,0,0,0,1'), dcnn_filter_size=[3] * len(dd), dcnn_depth=dd,
              dcnn_pool=s('2,1,2,1,2,1,2,1,2,1,1'), dcnn_skip_mask=m('1,0,1,0,1,0,0,0,0,1'), weight_decay=5e-5, use_bn=True,
              segm_loss_fn='bce', rnd_hflip=False, rnd_vflip=False, rnd_transpose=False, rnd_colour=False, add_skip_conn=True,
              base_learn_rate=1e-3, learn_rate_decay=0.96, steps_per_learn_rate_decay=5000, add_orientation=True,
              num_orientation_classes=8, num_semantic_classes=1, optimizer='momentum')


def cityscapes_opt():
  """run_cityscapes.sh:9-31."""
  s = lambda t: [int(v) for v in t.split(',')]
  m = lambda t: [v == '1' for v in t.split(',')]
  cd, dd = s('64,96,96,128,128,192,192,256,256,256,256,256,256,256,256,512,512,512,512,512'), s('512,512,256,256,192,192,128,128,96,96,64,64,17')
  return dict(inp_depth=3, padding=16, cnn_filter_size=[3] * len(cd), cnn_depth=cd,
              cnn_pool=s('1,2,1,2,1,2,1,2,1,1,1,1,1,1,1,2,1,1,1,2'), cnn_skip_mask=m('1,0,1,0,1,0,1,0,1,0,0,0,0,0,0,0,0,1,0,0,0'),
              dcnn_filter_size=[3] * len(dd), dcnn_depth=dd, dcnn_pool=s('2,1,2,1,2,1,2,1,2,1,2,1,1'),
              dcnn_skip_mask=m('1,0,1,0,1,0,1,0,1,0,1,0,0'), weight_decay=5e-5, use_bn=True, segm_loss_fn='bce', rnd_hflip=False,
              rnd_vflip=False, rnd_transpose=False, rnd_colour=False, add_skip_conn=True, base_learn_rate=0.01, learn_rate_decay=0.8,
              steps_per_learn_rate_decay=10000, add_orientation=True, num_orientation_classes=8, num_semantic_classes=9,
              optimizer='momentum')


def reduced_opt(nsc=1, orientation=True, wide=False):
  """A small net with every feature: pools 1 and 2, skips of the image and of two inner maps."""
  no = 8 if orientation else 0
  cd = [8, 16, 16, 144 if wide else 24, 24]
  dd = [16, 16, 12, 8, nsc + no]
  return dict(inp_depth=3, cnn_filter_size=[5] * 5, cnn_depth=cd, cnn_pool=[1, 2, 1, 2, 1], cnn_skip_mask=[True, False, True, False, True],
              dcnn_filter_size=[3] * 5, dcnn_depth=dd, dcnn_pool=[1, 2, 1, 2, 1], dcnn_skip_mask=[True, True, False, True],
              use_bn=True, add_skip_conn=True, add_orientation=orientation, num_orientation_classes=8, num_semantic_classes=nsc,
              weight_decay=5e-5)


def wiring(opt):
  """(cnn channels, dcnn channels, skip source per dcnn layer as an index into [x] + h_cnn or None) — fg_model.py:112-157."""
  cnn_ch = [opt['inp_depth']] + list(opt['cnn_depth'])
  n = len(opt['cnn_depth'])
  nd = len(opt['dcnn_filter_size'])
  dcnn_ch = [cnn_ch[-1]] + list(opt['dcnn_depth'])
  src = [None] * nd
  if opt.get('add_skip_conn'):
    if 'cnn_skip_mask' in opt:
      cmask = opt['cnn_skip_mask']
    elif 'cnn_skip' in opt:
      cmask = opt['cnn_skip']
    else:
      cmask = [True] * n
    dmask = opt['dcnn_skip_mask'] if 'dcnn_skip_mask' in opt else cmask[::-1]
    layers = []
    for k, sk in zip(range(n), cmask):  # zip over [x] + h_cnn[:-1]: n maps
      if sk:
        layers.append(k)
    src, counter = [None], len(layers) - 1
    for sk in dmask:
      if sk:
        src.append(layers[counter])
        counter -= 1
      else:
        src.append(None)
    src = (src + [None] * nd)[:nd]
  return cnn_ch, dcnn_ch, src


def dcnn_in_widths(opt):
  cnn_ch, dcnn_ch, src = wiring(opt)
  return [dcnn_ch[i] + (0 if src[i] is None else cnn_ch[src[i]]) for i in range(len(src))]


def weight_shapes(opt):
  """Checkpoint name -> shape (get_save_var, fg_model.py:270-285; filters as nnlib.py:202, :321)."""
  cnn_ch, dcnn_ch, _ = wiring(opt)
  win = dcnn_in_widths(opt)
  out = {}
  for i in range(len(cnn_ch) - 1):
    out['cnn/layer_%d/w' % i] = (3, 3, cnn_ch[i], cnn_ch[i + 1])
    out['cnn/layer_%d/b' % i] = (cnn_ch[i + 1],)
    if opt.get('use_bn', True):
      for k in BN:
        out['cnn/layer_%d/bn/%s' % (i, k)] = (cnn_ch[i + 1],)
  nd = len(dcnn_ch) - 1
  for i in range(nd):
    f = opt['dcnn_filter_size'][i]
    out['dcnn/layer_%d/w' % i] = (f, f, dcnn_ch[i + 1], win[i])
    out['dcnn/layer_%d/b' % i] = (dcnn_ch[i + 1],)
    if opt.get('use_bn', True) and i < nd - 1:
      for k in BN:
        out['dcnn/layer_%d/bn/%s' % (i, k)] = (dcnn_ch[i + 1],)
  return out


def random_weights(opt, seed):
  """He-scaled filters, BN statistics near (0, 1): activations keep their scale through 30 layers."""
  rng = np.random.RandomState(seed)
  P = {}
  for name, shp in sorted(weight_shapes(opt).items()):
    leaf = name.rsplit('/', 1)[1]
    if leaf == 'w':
      fan_in = shp[0] * shp[1] * (shp[3] if name.startswith('dcnn') else shp[2])
      P[name] = rng.randn(*shp) * np.sqrt(2.0 / fan_in)
    elif leaf == 'b':
      P[name] = rng.normal(0, 0.05, shp)
    elif leaf == 'beta':
      P[name] = rng.normal(0.05, 0.1, shp)
    elif leaf == 'gamma':
      P[name] = rng.uniform(0.9, 1.2, shp)
    elif leaf == 'ema_mean':
      P[name] = rng.normal(0, 0.1, shp)
    else:
      P[name] = rng.uniform(0.8, 1.2, shp)
    P[name] = P[name].astype(np.float32)
  return P


def quantise(v):
  """The 8-bit round trip: (v * 255).astype('uint8') written as PNG (fg_model_pack.py:41-48), read back as
  uint8.astype('float32') / 255 (data_api/ins_seg_dataset.py:273-292)."""
  return (np.asarray(v) * 255).astype('uint8').astype('float32') / np.float32(255)


def forward(opt, P, x):
  """float64 NumPy: {'logits', 'y_out', 'd_out' (None without orientation)}; x [B,H,W,inp_depth]."""
  f8 = lambda a: np.asarray(a, np.float64)
  cnn_ch, dcnn_ch, src = wiring(opt)
  bn = opt.get('use_bn', True)
  h = f8(x)
  maps = [h]
  for i in range(len(cnn_ch) - 1):
    h = ora.conv2d(h, f8(P['cnn/layer_%d/w' % i])) + f8(P['cnn/layer_%d/b' % i])
    if bn:
      h = ora.batch_norm_eval(h, *[f8(P['cnn/layer_%d/bn/%s' % (i, k)]) for k in BN])
    h = ora.relu(h)
    if opt['cnn_pool'][i] > 1:
      h = ora.max_pool(h, opt['cnn_pool'][i])
    maps.append(h)
  nd = len(dcnn_ch) - 1
  for i in range(nd):
    if src[i] is not None:
      h = np.concatenate([h, maps[src[i]]], axis=3)
    h = ora.conv2d_transpose(h, f8(P['dcnn/layer_%d/w' % i]), opt['dcnn_pool'][i]) + f8(P['dcnn/layer_%d/b' % i])
    if i < nd - 1:
      if bn:
        h = ora.batch_norm_eval(h, *[f8(P['dcnn/layer_%d/bn/%s' % (i, k)]) for k in BN])
      h = ora.relu(h)
  nsc = opt.get('num_semantic_classes', 1)
  ori = opt.get('add_orientation', False)
  want = nsc + (opt['num_orientation_classes'] if ori else 0)
  if h.shape[3] != want:
    raise ValueError('Expecting last channel to be %d' % want)
  y = h[..., :nsc] if ori else h
  d_out = ora.softmax(h[..., nsc:]) if ori else None
  y_out = ora.sigmoid(y) if nsc == 1 else ora.softmax(y)
  return dict(logits=h, y_out=y_out, d_out=d_out)


def forward_torch(opt, P, x):
  """The same net written again from the reference on torch CPU float64, channels first."""
  import torch
  import torch.nn.functional as F
  t = lambda a: torch.from_numpy(np.asarray(a, np.float64))
  ncnn, nd = len(opt['cnn_depth']), len(opt['dcnn_depth'])
  has_bn = opt.get('use_bn', True)

  def bnorm(h, pre):
    beta, gamma, mean, var = [t(P['%s/bn/%s' % (pre, k)]).view(1, -1, 1, 1) for k in BN]
    return (h - mean) * (gamma * torch.rsqrt(var + 1e-3)) + beta

  h = t(x).permute(0, 3, 1, 2)
  h_cnn = []
  inp = h
  for i in range(ncnn):
    pre = 'cnn/layer_%d' % i
    h = F.conv2d(h, t(P[pre + '/w']).permute(3, 2, 0, 1), t(P[pre + '/b']), padding=1)  # 3x3 SAME
    if has_bn:
      h = bnorm(h, pre)
    h = torch.relu(h)
    r = opt['cnn_pool'][i]
    if r > 1:
      h = F.max_pool2d(h, r, r)
    h_cnn.append(h)
  # fg_model.py:131-153
  skips = [None] * nd
  if opt.get('add_skip_conn'):
    mask = opt['cnn_skip_mask'] if 'cnn_skip_mask' in opt else (opt['cnn_skip'] if 'cnn_skip' in opt else [True] * ncnn)
    dmask = opt['dcnn_skip_mask'] if 'dcnn_skip_mask' in opt else mask[::-1]
    chosen = [hh for sk, hh in zip(mask, [inp] + h_cnn[:-1]) if sk]
    lst = [None]
    for sk in dmask:
      lst.append(chosen.pop() if sk else None)
    skips = (lst + [None] * nd)[:nd]
  for i in range(nd):
    pre = 'dcnn/layer_%d' % i
    if skips[i] is not None:
      h = torch.cat([h, skips[i]], dim=1)
    w = t(P[pre + '/w'])  # [f, f, out, in] -> conv_transpose2d's [in, out, f, f]
    f, s = w.shape[0], opt['dcnn_pool'][i]
    # TF SAME for the forward conv of size n*s: total padding max(f - s, 0), the smaller half first
    tot = max(f - s, 0)
    lo = tot // 2
    full = F.conv_transpose2d(h, w.permute(3, 2, 0, 1), None, stride=s)  # size (n - 1) s + f
    Ho, Wo = h.shape[2] * s, h.shape[3] * s
    full = F.pad(full, (0, max(0, lo + Wo - full.shape[3]), 0, max(0, lo + Ho - full.shape[2])))
    h = full[:, :, lo:lo + Ho, lo:lo + Wo] + t(P[pre + '/b']).view(1, -1, 1, 1)
    if i < nd - 1:
      if has_bn:
        h = bnorm(h, pre)
      h = torch.relu(h)
  h = h.permute(0, 2, 3, 1)
  nsc = opt.get('num_semantic_classes', 1)
  ori = opt.get('add_orientation', False)
  y = h[..., :nsc] if ori else h
  d_out = torch.softmax(h[..., nsc:], dim=-1).numpy() if ori else None
  y_out = torch.sigmoid(y) if nsc == 1 else torch.softmax(y, dim=-1)
  return dict(logits=h.contiguous().numpy(), y_out=y_out.numpy(), d_out=d_out)
