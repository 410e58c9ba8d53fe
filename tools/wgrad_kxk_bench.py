#!/usr/bin/env python
"""Per-layer time of the filter gradient for filter sizes 1 / 5 / 7 (ra_convkxk_wgrad_f32, csrc/ra_wgrad_kxk.hip) beside the 3x3
filter gradient (ra_conv3x3_wgrad_f32) at the same shape:  wgrad_kxk_bench.py [reps] [--out FILE]
Shapes: the layers of profiles/conv_filter_sizes.txt (tools/filter_size_bench.py) — cfg2's controller-CNN layers (CVPPP,
512 x 512) and the 48 x 48 patch layers of its attention CNN / DCNN, B = 8; the filter gradient runs on the conv's own map (before
the pool).  Device events around `reps` back-to-back launches after a warm-up; one row per layer: us per launch for each size and
its ratio to the 3x3 time, beside KF^2 / 9 (the ratio of the MFMA work) and the 1.5 x KF^2 / 9 the tap split is expected to stay
within.  Writes profiles/wgrad_filter_sizes.txt (or FILE)."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '..', 'rec-attend-public_amd'))
import numpy as np
import torch

import ra_native as rn
import ra_ops as ops

B = 8
# tools/filter_size_bench.py's layers: (name, H of x, Cin, Cout, pool, transposed stride or 0)
LAYERS = [('ctrl L0 4->8', 512, 4, 8, 1, 0), ('ctrl L1 8->8 p2', 512, 8, 8, 2, 0), ('ctrl L2 8->16', 256, 8, 16, 1, 0),
          ('ctrl L3 16->16 p2', 256, 16, 16, 2, 0), ('ctrl L4 16->32', 128, 16, 32, 1, 0),
          ('ctrl L5 32->32 p2', 128, 32, 32, 2, 0), ('ctrl L6 32->64 p2', 64, 32, 64, 2, 0),
          ('ctrl L7 64->64 p2', 32, 64, 64, 2, 0),
          ('attn L0 4->8', 48, 4, 8, 1, 0), ('attn L1 8->8 p2', 48, 8, 8, 2, 0), ('attn L2 8->16', 24, 8, 16, 1, 0),
          ('attn L3 16->16 p2', 24, 16, 16, 2, 0), ('attn L4 16->32', 12, 16, 32, 1, 0), ('attn L5 32->32 p2', 12, 32, 32, 2, 0),
          ('dcnn L0 32->32 s2', 3, 32, 32, 1, 2), ('dcnn L2 32->16 s2', 6, 32, 16, 1, 2), ('dcnn L4 16->8 s2', 12, 16, 8, 1, 2),
          ('dcnn L5 8->8', 24, 8, 8, 1, 1), ('dcnn L6 8->1 (48x48)', 48, 8, 1, 1, 1)]


def time_us(fn, reps):
  for _ in range(5):
    fn()
  torch.cuda.synchronize()
  e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  e0.record()
  for _ in range(reps):
    fn()
  e1.record()
  torch.cuda.synchronize()
  return e0.elapsed_time(e1) * 1e3 / reps


def main():
  args = [a for a in sys.argv[1:]]
  out = os.path.join(HERE, '..', 'profiles', 'wgrad_filter_sizes.txt')
  if '--out' in args:
    i = args.index('--out')
    out = args[i + 1]
    del args[i:i + 2]
  reps = int(args[0]) if args else 100
  if not torch.cuda.is_available():
    raise SystemExit('wgrad_kxk_bench.py needs an MI355X')
  dev = torch.device('cuda:0')
  lib = rn.lib()
  rng = np.random.RandomState(0)
  lines = ['# Filter gradient per layer for filter sizes 1 / 3 / 5 / 7 on one MI355X: python tools/wgrad_kxk_bench.py %d' % reps,
           '# 1x1, 5x5, 7x7: ra_convkxk_wgrad_f32 (csrc/ra_wgrad_kxk.hip: one tap row per workgroup slice, KF + 1 accumulator rows); 3x3:',
           '# ra_conv3x3_wgrad_f32 as its chooser dispatches it (csrc/ra_wgrad.hip).  The layers of profiles/conv_filter_sizes.txt, B = %d;' % B,
           '# the gradient runs on the conv\'s own map (before the pool).  Both launches of an entry (partial sums, finishing) are timed.',
           '# us per launch (%d launches after warm-up); (x) = time / 3x3 time; KF^2/9 = 0.11 / 1 / 2.78 / 5.44; expected within 1.5 x: 0.17 / - / 4.17 / 8.17'
           % reps,
           '%-22s %6s %15s %9s %15s %15s  %s' % ('layer', 'H', '1x1', '3x3', '5x5', '7x7', 'NT, grid of 7x7')]
  over = []
  for name, Hs, cin, cout, pool, tstride in LAYERS:
    ups = int(tstride == 2)
    H = Hs * (1 + ups)
    x = torch.tensor(rng.rand(B, Hs, Hs, cin).astype(np.float32), device=dev)
    du = torch.tensor(rng.randn(B, H, H, cout).astype(np.float32), device=dev)
    t = {}
    for kf in (1, 3, 5, 7):
      nws = lib.ra_convkxk_wgrad_workspace_floats(kf, cin, cout, B, H, H)
      ws = torch.empty(nws, device=dev)
      dw, db = torch.empty(kf, kf, cin, cout, device=dev), torch.empty(cout, device=dev)
      t[kf] = time_us(lambda: rn.check(lib.ra_convkxk_wgrad_f32(rn.ptr(x), cin, B, Hs, Hs, ups, rn.ptr(du), cout, kf, rn.ptr(ws), nws,
                                                                rn.ptr(dw), rn.ptr(db), rn.stream_ptr()), 'ra_convkxk_wgrad_f32'), reps)
    p = ops.wgrad_kxk_plan(7, cin, cout, B, H, H)
    cell = lambda kf: '%7.1f (%4.2f)' % (t[kf], t[kf] / t[3])
    lines.append('%-22s %6d %15s %9.1f %15s %15s  NT %d, %d x %d x %d' % (name, H, cell(1), t[3], cell(5), cell(7), p['nt'], p['grid_x'],
                                                                        p['grid_y'], p['grid_z']))
    over += ['%s %dx%d %.2f' % (name, kf, kf, t[kf] / t[3]) for kf in (1, 5, 7) if t[kf] / t[3] > 1.5 * kf * kf / 9.0]
  lines.append('# above 1.5 x KF^2/9 of the 3x3 time: %s' % ('; '.join(over) if over else 'none'))
  text = '\n'.join(lines) + '\n'
  sys.stdout.write(text)
  os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
  with open(out, 'w') as f:
    f.write(text)


if __name__ == '__main__':
  main()
