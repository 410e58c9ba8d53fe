#!/usr/bin/env python
"""Times the evaluator from instance-id images (csrc/ra_instance_eval.hip) against what the parent commit offers for the same
numbers, in one process (profiles/ins_eval.txt).

256 x 512 -> 1024 x 2048, T = 20, K = 1 and K = 10 thresholds, plain and with a foreground (mask + 5 x 5 dilation), B = 1, and
B = 4 as the largest batch tried.
  (a) ops.instance_eval_counts -> ops.eval_metrics_from_counts: one counting pass for all thresholds, one metrics launch;
  (b) pp.upsample [-> pp.morph] -> pp.apply_one_label, then per threshold pp.apply_threshold [-> pp.mask_foreground] ->
      ops.eval_metrics against y_gt planes [B,T,H,W].  The planes are made on the device from gt_ids and inst_id BEFORE the
      clock starts: (b) is not charged for them, although a run of the parent commit would have to load or build them.
Both end in the same tensors (stats [B,13], inst [B,6,T], iou_pairwise [B,T,T] per threshold), which are compared.

(a) and (b) alternate for ROUNDS rounds; a round is the median of REPS calls timed one by one between device events after a
warm-up.  The condition printed at the end: (a)'s slowest round is faster than (b)'s fastest round."""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(HERE, '..', 'rec-attend-public_amd'), os.path.join(HERE, '..', 'oracle'), os.path.join(HERE, '..', 'tests')]
import ra_ops as ops  # noqa: E402
from utils import postprocess as pp  # noqa: E402

ROUNDS, REPS, WARM = 5, 11, 3


def timed_events(fn):
  ts = []
  for i in range(WARM + REPS):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    if i >= WARM:
      ts.append(a.elapsed_time(b) * 1e3)
  return float(np.median(ts))


def inputs(B, T, Hs, Ws, H, W):
  import fg_eval_oracle as feo
  rng = np.random.RandomState(B)
  conf = rng.uniform(0.3, 1.0, (B, T, 1, 1)).astype(np.float32)
  yc = feo.smooth_map(rng, B * T, Hs, Ws).reshape(B, T, Hs, Ws) * conf
  rr, cc = np.mgrid[0:H, 0:W].astype(np.float32)
  ids = np.zeros((B, H, W), np.int32)
  for b in range(B):
    for i in range(T + 2):  # two more instances than slots: their pixels land in column T
      cy, cx, rad = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(0.05, 0.2) * min(H, W)
      ids[b][(rr - cy) ** 2 + (cc - cx) ** 2 <= rad ** 2] = i + 1
  inst_id = np.tile(np.arange(1, T + 1, dtype=np.int32), (B, 1))
  fg = feo.disc_labels(rng, B, H, W, n_disc=12) > 0
  dev = lambda a, t: torch.from_numpy(np.ascontiguousarray(a, t)).cuda()
  return dev(yc, np.float32), dev(ids, np.int32), dev(inst_id, np.int32), dev(fg, np.uint8)


def case(B, T, Hs, Ws, H, W, K, with_fg):
  yc, ids, inst_id, fg8 = inputs(B, T, Hs, Ws, H, W)
  thr = [0.3] if K == 1 else [0.1 * k for k in range(K)]
  s_gt = torch.ones((B, T), dtype=torch.float32, device='cuda')
  y_gt = (ids[:, None] == inst_id[:, :, None, None]).to(torch.float32).contiguous()  # not charged to (b)
  fg8 = fg8 if with_fg else None
  fgf = fg8.to(torch.float32) if with_fg else None

  def fused():
    inter, area_b = ops.instance_eval_counts(yc, ids, inst_id, thr, fg=fg8, morph=with_fg, check_fg=False)
    return ops.eval_metrics_from_counts(inter, area_b, s_gt)

  def chain():
    v = pp.upsample(yc, (H, W))
    if with_fg:
      v = pp.morph(v)
    one = pp.apply_one_label(v)
    out = []
    for t in thr:
      y = pp.apply_threshold(one, t)
      if with_fg:
        y = pp.mask_foreground(y, fgf)
      out.append(ops.eval_metrics(y, y_gt, s_gt))
    return out

  a, b = fused(), chain()
  diff = max(float((x[k] - y[k]).abs().max()) for x, y in zip(a, b) for k in ('stats', 'inst', 'iou_pairwise'))
  del a, b
  ra, rb = [], []
  for _ in range(ROUNDS):
    ra.append(timed_events(fused))
    rb.append(timed_events(chain))
  px, plane = B * H * W, B * T * H * W * 4
  # (a): yc once from memory (the tiles re-read it from L2), 4 bytes of id and 1 of fg per pixel, the bins
  bytes_a = yc.numel() * 4 + px * (5 if with_fg else 4) + B * K * T * (T + 1) * 4
  # (b), in planes of B T H W floats: resize w, bilateral r + w, [dilate r + w], one-label r + w then r r w, and per threshold
  # compare r + w, [mask r + w], two unions r r, the main pair pass r r, the two union-against-planes passes r r
  bytes_b = yc.numel() * 4 + plane * (1 + 2 + (2 if with_fg else 0) + 5 + K * (2 + (2 if with_fg else 0) + 6))
  ok = max(ra) < min(rb)
  print('B=%d T=%d %dx%d->%dx%d K=%-2d %-9s (a) %9.1f us [%.1f .. %.1f]   (b) %10.1f us [%.1f .. %.1f]   x%.1f   (a) beats (b) beyond the '
        'spread: %s   max |metric(a) - metric(b)| %.2g   traffic model: (a) %.1f MB, (b) %.1f MB' % (
            B, T, Hs, Ws, H, W, K, 'fg+morph' if with_fg else 'plain', np.median(ra), min(ra), max(ra), np.median(rb), min(rb), max(rb),
            np.median(rb) / np.median(ra), ok, diff, bytes_a / 1e6, bytes_b / 1e6), flush=True)
  return ok


def main():
  p = argparse.ArgumentParser()
  p.add_argument('--small', action='store_true', help='a rehearsal at toy sizes (numbers mean nothing)')
  p.add_argument('--batches', default='1,4', help='batch sizes; (b) holds about 6 planes of B * T * H * W floats at a time')
  args = p.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit('ins_eval_bench needs an MI355X; there is nothing to time without one')
  print('rounds %d, calls per round %d (median), warm-up %d' % (ROUNDS, REPS, WARM))
  shape = (32, 64, 128, 256) if args.small else (256, 512, 1024, 2048)
  ok = True
  for B in [int(b) for b in args.batches.split(',')]:
    for K in (1, 10):
      for with_fg in (False, True):
        ok &= case(B, 20, *shape, K, with_fg)
  print('condition (a) beats (b) beyond the spread of the rounds, everywhere: %s' % ok)


if __name__ == '__main__':
  main()
