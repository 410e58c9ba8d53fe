#!/usr/bin/env python
"""Per-layer time of K1 for filter sizes 1 / 3 / 5 / 7 (ra_convkxk_f32; 3 = ra_conv3x3_f32 as the engine dispatches it):
filter_size_bench.py [reps].  Shapes: cfg2's controller-CNN layers (CVPPP, 512 x 512, B = 8) and the 48 x 48 patch layers of
its attention CNN / DCNN (B = 8).  Device events around `reps` back-to-back launches after a warm-up; prints one row per
layer, us per launch for each size and its ratio to the 3x3 time, beside KF^2 / 9 (the ratio of the MFMA work)."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'rec-attend-public_amd'))
import numpy as np
import torch

import ra_ops as ops

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 100
dev = torch.device('cuda:0')
B = 8
# (name, H, Cin, Cout, pool, transposed stride or 0)
LAYERS = [('ctrl L0 4->8', 512, 4, 8, 1, 0), ('ctrl L1 8->8 p2', 512, 8, 8, 2, 0), ('ctrl L2 8->16', 256, 8, 16, 1, 0),
          ('ctrl L3 16->16 p2', 256, 16, 16, 2, 0), ('ctrl L4 16->32', 128, 16, 32, 1, 0),
          ('ctrl L5 32->32 p2', 128, 32, 32, 2, 0), ('ctrl L6 32->64 p2', 64, 32, 64, 2, 0),
          ('ctrl L7 64->64 p2', 32, 64, 64, 2, 0),
          ('attn L0 4->8', 48, 4, 8, 1, 0), ('attn L1 8->8 p2', 48, 8, 8, 2, 0), ('attn L2 8->16', 24, 8, 16, 1, 0),
          ('attn L3 16->16 p2', 24, 16, 16, 2, 0), ('attn L4 16->32', 12, 16, 32, 1, 0), ('attn L5 32->32 p2', 12, 32, 32, 2, 0),
          ('dcnn L0 32->32 s2', 3, 32, 32, 1, 2), ('dcnn L2 32->16 s2', 6, 32, 16, 1, 2), ('dcnn L4 16->8 s2', 12, 16, 8, 1, 2),
          ('dcnn L5 8->8', 24, 8, 8, 1, 1), ('dcnn L6 8->1 (48x48)', 48, 8, 1, 1, 1)]


def time_us(fn):
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


if not torch.cuda.is_available():
  raise SystemExit('filter_size_bench.py needs an MI355X')
rng = np.random.RandomState(0)
print('# us per launch (B = %d, %d launches after warm-up); (x) = time / 3x3 time; KF^2/9 = 0.11 / 1 / 2.78 / 5.44' % (B, reps))
print('%-22s %9s %15s %9s %15s %15s' % ('layer', 'Hout', '1x1', '3x3', '5x5', '7x7'))
for name, H, cin, cout, pool, tstride in LAYERS:
  x = torch.tensor(rng.rand(B, H, H, cin).astype(np.float32), device=dev)
  cp = ops.cout_padded(cout)
  sc, sh = torch.ones(cp, device=dev), torch.zeros(cp, device=dev)
  Hout = H * (2 if tstride == 2 else 1) // pool
  y = torch.empty((B, Hout, Hout, cout), device=dev)
  t = {}
  for kf in (1, 3, 5, 7):
    shp = (kf, kf, cout, cin) if tstride else (kf, kf, cin, cout)
    wp = torch.tensor(ops.pack_conv_weights((rng.randn(*shp) * 0.1).astype(np.float32), transposed=bool(tstride)), device=dev)
    t[kf] = time_us(lambda: ops.conv2d_fused(x, wp, sc, sh, cout, kf, relu=True, pool=pool, upsample=(tstride == 2), out=y))
  cell = lambda kf: '%7.1f (%4.2f)' % (t[kf], t[kf] / t[3])
  print('%-22s %9d %15s %9.1f %15s %15s' % (name, Hout, cell(1), t[3], cell(5), cell(7)))
