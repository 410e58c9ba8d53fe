#!/usr/bin/env python
"""Time the fused conv pair (ra_conv_pair_f32) at given shapes: pair_shape_bench.py B,Hs,Ws,Cin,CoutA,CoutB,poolB,upsA [...]
prints, per shape, the plan the dispatch reports and us per launch in a HIP graph of 8 copies replayed 20 times (as
tools/pair8_probe.hip times its launch).  RA_LIB = another build of the library (same ABI) for a same-box A/B; the RA_PAIR*
variables pick the other kernels (RA_PAIR_PERSIST=0, RA_PAIR_NO8=1, RA_PAIR_GEO=<gx><gyb>)."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'rec-attend-public_amd'))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'tests'))
import numpy as np
import torch

import ra_native as rn
if os.environ.get('RA_LIB'):  # A/B: another build of the library (same ABI)
  rn.LIB_PATH = os.environ['RA_LIB']
import conv_form_cases as cf
import ra_ops as ops

COPIES, REPLAYS = 8, 20
dev = torch.device('cuda:0')
for arg in sys.argv[1:]:
  B, Hs, Ws, Ci, Ca, Cb, pool, ups = [int(v) for v in arg.split(',')]
  rng = np.random.RandomState(0)
  x = torch.tensor(rng.randn(B, Hs, Ws, Ci).astype(np.float32), device=dev)
  wA = (rng.randn(*((3, 3, Ca, Ci) if ups else (3, 3, Ci, Ca))) * 0.2).astype(np.float32)
  wB = (rng.randn(*((3, 3, Cb, Ca) if ups else (3, 3, Ca, Cb))) * 0.2).astype(np.float32)
  wpA, wpB = [torch.tensor(ops.pack_conv_weights(w, transposed=bool(ups)), device=dev) for w in (wA, wB)]
  sc, sh = torch.ones(32, device=dev), torch.zeros(32, device=dev)
  y = torch.empty((B, Hs * (1 + ups) // pool, Ws * (1 + ups) // pool, Cb), device=dev)
  launch = lambda: ops.conv_pair(x, wpA, sc, sh, Ca, wpB, sc, sh, Cb, poolB=pool, upsampleA=bool(ups), out=y)
  launch()
  torch.cuda.synchronize()
  g = torch.cuda.CUDAGraph()
  with torch.cuda.graph(g):
    for _ in range(COPIES):
      launch()
  for _ in range(3):
    g.replay()
  torch.cuda.synchronize()
  e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  e0.record()
  for _ in range(REPLAYS):
    g.replay()
  e1.record()
  torch.cuda.synchronize()
  us = e0.elapsed_time(e1) * 1e3 / (COPIES * REPLAYS)
  plan = cf.plan_str(ops.conv_pair_plan(Ci, B, Hs, Ws, Ca, Cb, poolB=pool, upsampleA=bool(ups)))
  print('pair %-26s %8.2f us   %s' % (arg, us, plan), flush=True)
