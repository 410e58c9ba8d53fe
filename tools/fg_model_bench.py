#!/usr/bin/env python
"""Times of the fg_model pre-stage on one MI355X: fg_model_bench.py [reps >= 21] [--out FILE].

Per distinct wide layer (more than 128 output channels: ra_conv3x3_wide_f32) of the nets of run_kitti.sh (128 x 448,
B = 8) and run_cityscapes.sh (256 x 512, B = 4): us per launch, algorithmic GFLOP (2 x 9 x Cin x Cout x conv pixels) and
the share of the 157.3 TF/s f32-MFMA peak.  Then the whole pre-stage (every layer and the head, prestage(quantise=True)):
ms per batch and per image, algorithmic GFLOP per image (20.2 / 107.2 from the shapes alone; the tool stops if it
arrives elsewhere).  Device events around every single launch after a warm-up, median of `reps`."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'rec-attend-public_amd'))
import numpy as np

import fg_model

PEAK_TF = 157.3  # f32 MFMA, the project's yardstick
_s = lambda t: [int(v) for v in t.split(',')]
_m = lambda t: [v == '1' for v in t.split(',')]


def net_opt(name):
  """The option lists of run_kitti.sh:13-28 / run_cityscapes.sh:9-31."""
  if name == 'kitti':
    cd, dd = _s('32,64,64,96,96,128,128,128,128,128,128,128,128,256,256,256,256,512'), _s('256,256,128,128,96,96,64,64,32,32,9')
    cp, dp = _s('1,2,1,2,1,2,1,1,1,1,1,1,1,2,1,1,1,2'), _s('2,1,2,1,2,1,2,1,2,1,1')
    cs, ds, nsc = _m('1,0,0,0,0,1,0,0,0,0,0,0,0,1,0,0,0,1'), _m('1,0,1,0,1,0,0,0,0,1'), 1
  else:
    cd, dd = _s('64,96,96,128,128,192,192,256,256,256,256,256,256,256,256,512,512,512,512,512'), _s('512,512,256,256,192,192,128,128,96,96,64,64,17')
    cp, dp = _s('1,2,1,2,1,2,1,2,1,1,1,1,1,1,1,2,1,1,1,2'), _s('2,1,2,1,2,1,2,1,2,1,2,1,1')
    cs, ds, nsc = _m('1,0,1,0,1,0,1,0,1,0,0,0,0,0,0,0,0,1,0,0,0'), _m('1,0,1,0,1,0,1,0,1,0,1,0,0'), 9
  return dict(inp_depth=3, cnn_filter_size=[3] * len(cd), cnn_depth=cd, cnn_pool=cp, cnn_skip_mask=cs, dcnn_filter_size=[3] * len(dd),
              dcnn_depth=dd, dcnn_pool=dp, dcnn_skip_mask=ds, use_bn=True, add_skip_conn=True, add_orientation=True,
              num_orientation_classes=8, num_semantic_classes=nsc)


def layers(d, H, W):
  """(kind, Hs, Ws, C0, C1, Cout, pool | stride, conv pixels) of every layer of a net described by fg_model.derive()."""
  out, h, w = [], H, W
  ch = d['cnn_channels']
  for i, p in enumerate(d['cnn_pool']):
    out.append(('conv', h, w, ch[i], 0, ch[i + 1], p, h * w))
    h, w = h // p, w // p
  dc = d['dcnn_channels']
  for i, s in enumerate(d['dcnn_pool']):
    c1 = d['dcnn_skip_ch'][i] if d['dcnn_skip_ch'] else 0
    out.append(('tconv', h, w, dc[i], c1, dc[i + 1], s, h * s * w * s))
    h, w = h * s, w * s
  return out


def gflop(layer):
  return 2.0 * 9 * (layer[3] + layer[4]) * layer[5] * layer[7] * 1e-9


def main():
  import torch
  import ra_ops as ops
  args = [a for a in sys.argv[1:] if not a.startswith('--')]
  reps = max(21, int(args[0])) if args else 31
  out_path = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else None
  if not torch.cuda.is_available():
    raise SystemExit('fg_model_bench.py needs an MI355X')
  dev = torch.device('cuda:0')
  lines = []

  def say(s):
    print(s, flush=True)
    lines.append(s)

  def median_us(fn):
    for _ in range(5):
      fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
      e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      e0.record()
      fn()
      e1.record()
      e1.synchronize()
      ts.append(e0.elapsed_time(e1) * 1e3)
    return float(np.median(ts))

  rng = np.random.RandomState(0)
  r4 = lambda c: -(-c // 4) * 4
  for name, H, W, B, want in (('kitti', 128, 448, 8, 20.2), ('cityscapes', 256, 512, 4, 107.2)):
    opt = net_opt(name)
    d = fg_model.derive(opt)
    L = layers(d, H, W)
    total = sum(gflop(l) for l in L)
    if abs(total - want) > 0.05:
      raise SystemExit('%s: %.2f algorithmic GFLOP per image, expected %.1f' % (name, total, want))
    say('# %s: %d x %d, B = %d; %.1f algorithmic GFLOP per image, %.1f of them in the wide layers; device events, median of %d' %
        (name, H, W, B, total, sum(gflop(l) for l in L if l[5] > 128), reps))
    say('%-44s %6s %10s %9s %9s' % ('wide layer (source map, channels)', 'count', 'us', 'GFLOP', '% of peak'))
    seen = {}
    for l in L:
      if l[5] > 128:
        seen[l[:7]] = seen.get(l[:7], 0) + 1
    wide_us = 0.0
    for key, count in seen.items():
      kind, hs, ws, c0, c1, cout, ps = key
      tr = kind == 'tconv'
      k0, k1 = r4(c0), r4(c1)
      x0 = torch.tensor(rng.randn(B, hs, ws, k0).astype(np.float32), device=dev)
      x1 = torch.tensor(rng.randn(B, hs, ws, k1).astype(np.float32), device=dev) if c1 else None
      wshape = (3, 3, cout, k0 + k1) if tr else (3, 3, k0 + k1, cout)
      wp = torch.tensor(ops.pack_wide_weights((rng.randn(*wshape) * 0.05).astype(np.float32), transposed=tr), device=dev)
      sc, sh = torch.ones(cout, device=dev), torch.zeros(cout, device=dev)
      up = tr and ps == 2
      pool = 1 if tr else ps
      y = torch.empty((B, hs * (2 if up else 1) // pool, ws * (2 if up else 1) // pool, cout), device=dev)
      us = median_us(lambda: ops.conv_wide(x0, wp, sc, sh, cout, relu=True, pool=pool, src1=x1, upsample=up, out=y))
      g = B * 2.0 * 9 * (c0 + c1) * cout * hs * ws * (4 if up else 1) * 1e-9
      wide_us += us * count
      label = '%s%s %dx%d %d%s -> %d' % (kind, (' s%d' % ps if tr else ' p%d' % ps), hs, ws, c0, '+%d' % c1 if c1 else '', cout)
      say('%-44s %6d %10.1f %9.2f %9.1f' % (label, count, us, g, 100 * g * 1e9 / (us * 1e-6) / (PEAK_TF * 1e12)))
    model = fg_model.get_model(opt)
    for k in model.weight_keys():
      leaf = k.rsplit('/', 1)[1]
      t = model[fg_model.save_var_names(model)[k]]
      if leaf == 'w':
        t.copy_(torch.randn(t.shape) * float(np.sqrt(2.0 / (9 * (t.shape[3] if k.startswith('dcnn') else t.shape[2])))))
      elif leaf in ('gamma', 'ema_var'):
        t.fill_(1.0)
    x = torch.tensor(rng.rand(B, H, W, 3).astype(np.float32), device=dev)
    us = median_us(lambda: model.prestage(x, quantise=True))
    say('whole pre-stage (%d layers + head): %.2f ms per batch, %.2f ms per image; %.1f %% of the f32-MFMA peak; '
        'wide layers alone %.2f ms per batch' % (len(L), us * 1e-3, us * 1e-3 / B, 100 * total * B * 1e9 / (us * 1e-6) / (PEAK_TF * 1e12),
                                                  wide_us * 1e-3))
    say('')
  if out_path:
    with open(out_path, 'w') as f:
      f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
  main()
