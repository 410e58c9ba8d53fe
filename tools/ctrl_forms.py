#!/usr/bin/env python
"""us per launch of the three controller forms (one workgroup per image, 16 per image, 16 per group of images), HIP-graph replay.

  python tools/ctrl_forms.py [--lib SO]            at cfg2 (B = 8) and cfg3 (B = 16, 8) shapes
  python tools/ctrl_forms.py --iters-sweep [B]     cfg2's shape over glimpse iterations / glimpse-MLP depth: the marginal cost of
                                                   an iteration and the fixed cost of a launch (RA_CTRL_XCD=0: the agent-scope exchange)

--lib times another build of librecattend.so (same ABI) from this tree: a same-box A/B in alternating fresh processes."""
import argparse
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'rec-attend-public_amd')]
import torch
import ra_native as rn


def t_us(fn, reps=50):
  fn(); torch.cuda.synchronize()
  g = torch.cuda.CUDAGraph()
  with torch.cuda.graph(g):
    for _ in range(8):
      fn()
  for _ in range(3):
    g.replay()
  e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  torch.cuda.synchronize(); e0.record()
  for _ in range(reps):
    g.replay()
  e1.record(); torch.cuda.synchronize()
  return 1e3 * e0.elapsed_time(e1) / (reps * 8)


ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
ap.add_argument('--lib', help='the librecattend.so to time (default: the tree\'s own)')
ap.add_argument('--iters-sweep', type=int, nargs='?', const=8, metavar='B')
args = ap.parse_args()
if args.lib:
  rn.LIB_PATH = os.path.abspath(args.lib)
import bench, full_model, ra_ops as ops
shapes = [('cvppp', 512, 512, 8, {}), ('kitti', 128, 448, 16, {}), ('kitti', 128, 448, 8, {})]
if args.iters_sweep is not None:
  shapes = [('cvppp', 512, 512, args.iters_sweep, {'num_ctrl_rnn_iter': it, 'num_glimpse_mlp_layers': ng})
            for it, ng in ((1, 2), (2, 2), (3, 2), (5, 2), (5, 1))]
for arch, H, W, B, over in shapes:
  opt = bench.make_opt(arch, H, W, 4)
  opt.update(over)
  m = full_model.get_model(opt, is_training=False)
  bench.seed_weights(m, 1)
  e = m.engine
  e.prepare(torch.device('cuda'))
  d, Wt = m.dims, e.W
  feat = torch.rand(B, d['G'], d['ccnn_channels'][-1], device='cuda')
  z = lambda *s: torch.zeros(s, device='cuda')
  h, co, gm, at = z(B, d['hid']), z(B, 9), z(B, d['iters'], d['G']), z(B, 16)
  out = ['%s %dx%d B=%d iters=%d n_gmlp=%d:' % (arch, H, W, B, d['iters'], d['n_gmlp'])]
  out.append('one-workgroup %.1f' % t_us(lambda: ops.controller(e.desc, feat, Wt['ctrl'], h, co, gm, at)))
  if B <= 14:
    ws, st = ops.ctrl_split_workspace(e.desc, B, 'cuda')
    out.append('split %.1f (status %d)' % (t_us(lambda: ops.controller_split(e.desc, feat, Wt['ctrl_split'], h, co, gm, at, ws, st)), int(st.item())))
  if ops.ctrl_batch_supported(e.desc):
    ws, st = ops.ctrl_batch_workspace(e.desc, B, 'cuda')
    out.append('group-shared %.1f (status %d)' % (t_us(lambda: ops.controller_batch(e.desc, feat, Wt['ctrl_split'], h, co, gm, at, ws, st)), int(st.item())))
  print(' | '.join(out), flush=True)
