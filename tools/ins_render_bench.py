#!/usr/bin/env python
"""Times the pictures of the evaluator's id path (csrc/ra_instance_eval.hip's winner map + csrc/ra_instance_paint.hip) against
what the parent commit offers for the same pictures, in one process (profiles/ins_render.txt).

256 x 512 -> 1024 x 2048, T = 20, B in {1, 4}, K in {1, 10} thresholds, plain and with a foreground (mask + 5 x 5 dilation +
remove_tiny): the shape and the inputs of tools/ins_eval_bench.py.
  (a) ops.instance_eval_counts(..., want_map=True) -> ops.eval_metrics_from_counts -> ops.paint_instances(keep=paint_keep):
      K pictures [K,B,H,W,3] from one counting pass;
  (b) the plane chain of utils/postprocess.py — pp.upsample [-> pp.morph] -> pp.apply_one_label, then per threshold
      pp.apply_threshold [-> pp.mask_foreground -> pp.remove_tiny] — followed by ops.render_instances: K pictures [B,H,W,3];
  (c) the counting pass alone, without and with the map output, to show what the map costs it.
The pictures of (a) and (b) are compared and the differing pixels counted.

The forms alternate for ROUNDS rounds; a round is the median of REPS calls timed one by one between device events after a
warm-up.  The only condition stated and checked: (a)'s slowest round is faster than (b)'s fastest round, in every row.  (c)
is reported as found."""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(HERE, '..', 'rec-attend-public_amd'), os.path.join(HERE, '..', 'oracle'), os.path.join(HERE, '..', 'tests'), HERE]
import ra_ops as ops  # noqa: E402
from ins_eval_bench import ROUNDS, REPS, WARM, inputs, timed_events  # noqa: E402
from utils import postprocess as pp  # noqa: E402

REMOVE_TINY = 400


def case(B, T, Hs, Ws, H, W, K, with_fg, emit):
  yc, ids, inst_id, fg8 = inputs(B, T, Hs, Ws, H, W)
  thr = [0.3] if K == 1 else [0.1 * k for k in range(K)]
  s_gt = torch.ones((B, T), dtype=torch.float32, device='cuda')
  conf = torch.ones((B, T), dtype=torch.float32, device='cuda')
  fg8 = fg8 if with_fg else None
  fgf = fg8.to(torch.float32) if with_fg else None
  tiny = REMOVE_TINY if with_fg else 0

  def painted():
    inter, area_b, wmap = ops.instance_eval_counts(yc, ids, inst_id, thr, fg=fg8, morph=with_fg, check_fg=False, want_map=True)
    per = ops.eval_metrics_from_counts(inter, area_b, s_gt, remove_tiny=tiny, conf=conf)
    return ops.paint_instances(wmap, thr, keep=ops.paint_keep(per))

  def chain():
    v = pp.upsample(yc, (H, W))
    if with_fg:
      v = pp.morph(v)
    one = pp.apply_one_label(v)
    out = []
    for t in thr:
      y = pp.apply_threshold(one, t)
      if with_fg:
        y, _ = pp.remove_tiny(pp.mask_foreground(y, fgf), conf, threshold=tiny)
      out.append(ops.render_instances(y.contiguous()))
    return out

  plain = lambda: ops.instance_eval_counts(yc, ids, inst_id, thr, fg=fg8, morph=with_fg, check_fg=False)
  mapped = lambda: ops.instance_eval_counts(yc, ids, inst_id, thr, fg=fg8, morph=with_fg, check_fg=False, want_map=True)

  a, b = painted(), chain()
  differ = sum(int((a[k] != b[k]).any(dim=-1).sum()) for k in range(K))
  del a, b
  ra, rb, rc, rm = [], [], [], []
  for _ in range(ROUNDS):
    ra.append(timed_events(painted))
    rb.append(timed_events(chain))
    rc.append(timed_events(plain))
    rm.append(timed_events(mapped))
  px = B * H * W
  # the map: 2 bytes per pixel out of the counting pass; paint: 2 bytes in and 3 * K out per pixel
  mb_map, mb_paint = px * 2 / 1e6, px * (2 + 3 * K) / 1e6
  ok = max(ra) < min(rb)
  emit('%-2d %-3d %-9s %9.1f %9.1f ..%9.1f  %10.1f %10.1f ..%10.1f  %6.1f  %-5s %9.1f %9.1f ..%9.1f  %9.1f %9.1f ..%9.1f  %8.1f  %8.1f  %d of %d' % (
      B, K, 'fg+morph' if with_fg else 'plain', np.median(ra), min(ra), max(ra), np.median(rb), min(rb), max(rb), np.median(rb) / np.median(ra),
      'yes' if ok else 'NO', np.median(rc), min(rc), max(rc), np.median(rm), min(rm), max(rm), mb_map, mb_paint, differ, K * px))
  return ok


def main():
  p = argparse.ArgumentParser()
  p.add_argument('--small', action='store_true', help='a rehearsal at toy sizes (numbers mean nothing)')
  p.add_argument('--batches', default='1,4', help='batch sizes; (b) holds about 6 planes of B * T * H * W floats at a time')
  p.add_argument('--out', default=None, help='also write the table to this file')
  args = p.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit('ins_render_bench needs an MI355X; there is nothing to time without one')
  lines = []

  def emit(s):
    print(s, flush=True)
    lines.append(s)

  shape = (32, 64, 128, 256) if args.small else (256, 512, 1024, 2048)
  emit('# rounds %d, calls per round %d (median), warm-up %d; T = 20, %d x %d -> %d x %d; times in us, [min .. max] over the rounds' % (
      (ROUNDS, REPS, WARM) + shape))
  emit('# (a) counts with map + eval_metrics_from_counts + paint_instances   (b) plane chain + render_instances per threshold')
  emit('# (c) the counting pass alone, without / with the map output; model MB: the map (2 B per pixel out), paint (2 B in, 3 K out)')
  emit('B  K   form         (a) med    (a) min ..  (a) max     (b) med    (b) min ..   (b) max  (b)/(a) a<b    (c) no map    min ..      max   (c) map       min ..      max    map MB  paint MB  pixels that differ (a) vs (b)')
  ok = True
  for B in [int(b) for b in args.batches.split(',')]:
    for K in (1, 10):
      for with_fg in (False, True):
        ok &= case(B, 20, *shape, K, with_fg, emit)
  emit('# condition "(a)\'s slowest round beats (b)\'s fastest round" in every row: %s' % ok)
  if args.out:
    with open(args.out, 'w') as f:
      f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
  main()
