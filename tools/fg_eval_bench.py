#!/usr/bin/env python
"""Times the two kernels of csrc/ra_fg_eval.hip against what the ops of the parent commit offer for the same numbers, in one
process (profiles/fg_eval.txt).

sweep   K = 10 thresholds, 256 x 512 -> 1024 x 2048, B = 1 and B = 4.
        (a) ops.fg_sweep_counts_device: the fused kernel;
        (b) ops.resize_linear -> ops.bilateral5 -> per threshold compare, product with gt and the two sums (torch), + sum(gt).
stats   256 x 512, B = 1 and 4, nsc 9 + 8 orientation classes (run_cityscapes.sh) and 1 + 8 (run_kitti.sh).
        (a) ops.fg_statistics (its copy of nine doubles to the host included: it is part of the call);
        (b) ops.fg_head, then the six statistics of fg_model.py:196-246 with torch ops on y_out / d_out, copied to the host.

(a) and (b) alternate for ROUNDS rounds; a round is the median of REPS launches timed one by one between device events (for
the statistics: a host clock around the call, which ends in a synchronising copy) after a warm-up.  The condition printed at
the end: (a)'s slowest round is faster than (b)'s fastest round.  The counters / statistics of (a) and (b) are compared."""
import argparse
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(HERE, '..', 'rec-attend-public_amd'), os.path.join(HERE, '..', 'oracle'), os.path.join(HERE, '..', 'tests')]
import ra_ops as ops  # noqa: E402

ROUNDS, REPS, WARM = 5, 21, 5


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


def timed_host(fn):
  ts = []
  for i in range(WARM + REPS):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()  # ends in a copy to the host
    if i >= WARM:
      ts.append((time.perf_counter() - t0) * 1e6)
  return float(np.median(ts))


def alternate(fa, fb, timer):
  ra, rb = [], []
  for _ in range(ROUNDS):
    ra.append(timer(fa))
    rb.append(timer(fb))
  return ra, rb


def report(what, ra, rb, extra=''):
  ok = max(ra) < min(rb)
  print('%-34s (a) %8.1f us [%.1f .. %.1f]   (b) %8.1f us [%.1f .. %.1f]   x%.1f   (a) beats (b) beyond the spread: %s%s' % (
      what, np.median(ra), min(ra), max(ra), np.median(rb), min(rb), max(rb), np.median(rb) / np.median(ra), ok, extra))
  return ok


def sweep(B, Hs, Ws, H, W, K):
  import fg_eval_oracle as feo
  rng = np.random.RandomState(B)
  src = torch.from_numpy(feo.smooth_map(rng, B, Hs, Ws)).cuda()
  gt = torch.from_numpy(feo.disc_labels(rng, B, H, W, n_disc=12)).cuda()
  thr = [0.1 * k for k in range(K)]
  out = torch.empty((B, ops.rn.RA_FG_SWEEP_SLOTS), dtype=torch.int64, device='cuda')
  g64 = gt.to(torch.int64)

  def fused():
    return ops.fg_sweep_counts_device(src, gt, thr, out=out)

  def chain():
    v = ops.bilateral5(ops.resize_linear(src, H, W))
    ca, sab = [], []
    for t in thr:
      m = v > t
      ca.append(m.sum(dim=(1, 2)))
      sab.append((m * gt).sum(dim=(1, 2)))
    return torch.stack(ca, 1), torch.stack(sab, 1), g64.sum(dim=(1, 2))

  c = fused().cpu().numpy()
  ca, sab, sb = [t.cpu().numpy() for t in chain()]
  same = (c[:, :K] == ca).all() and (c[:, 16:16 + K] == sab).all() and (c[:, 32] == sb).all()
  diff = int(np.abs(c[:, :K] - ca).sum() + np.abs(c[:, 16:16 + K] - sab).sum())
  ra, rb = alternate(fused, chain, timed_events)
  hw = B * H * W
  model = '   traffic model: (a) %.1f MB, (b) %.1f MB' % ((hw + B * Hs * Ws * 4) / 1e6, (B * Hs * Ws * 4 + 4 * hw + 8 * hw + K * 10 * hw + 8 * hw) / 1e6)
  return report('sweep B=%d %dx%d->%dx%d K=%d' % (B, Hs, Ws, H, W, K), ra, rb, '   counters equal: %s (sum |diff| %d)%s' % (same, diff, model))


def stats(B, H, W, nsc, no):
  rng = np.random.RandomState(B + nsc)
  lg = torch.from_numpy((rng.randn(B, H, W, nsc + no) * 2.5).astype(np.float32)).cuda()
  if nsc == 1:
    g = torch.from_numpy((rng.rand(B, H, W, 1) > 0.6).astype(np.float32)).cuda()
  else:
    g = torch.from_numpy(np.eye(nsc, dtype=np.float32)[rng.randint(0, nsc, (B, H, W))]).cuda()
  d = torch.from_numpy(np.eye(8, dtype=np.float32)[rng.randint(0, 8, (B, H, W))]).cuda()
  npix = float(B * H * W)

  def fused():
    s = ops.fg_statistics(lg, g, d, nsc, no)
    iou = lambda i, a, b: i / (a + b - i + 1e-5)
    return [iou(s['inter_soft'], s['sum_soft'], s['sum_gt']), iou(s['inter_hard'], s['sum_hard'], s['sum_gt']), s['seg_ce'] / npix,
            s['ori_ce'] / s['mask'], s['ori_correct'] / s['mask']]

  def torch_ops():  # fg_model.py:196-246 on the head's outputs
    y, dd = ops.fg_head(lg, nsc, no)
    if nsc == 1:
      mask, hard, ys, gs = g, (y > 0.5).float(), y, g
      seg = (-g * torch.log(y + 1e-5) - (1 - g) * torch.log(1 - y + 1e-5)).sum()
    else:
      mask = g[..., 1:].max(dim=3, keepdim=True).values
      hard = (y == y.max(dim=3, keepdim=True).values).float()[..., 1:]
      ys, gs = y[..., 1:], g[..., 1:]
      seg = (-g * torch.log(y + 1e-5)).sum()
    iou = lambda a, b: (a * b).sum() / (a.sum() + b.sum() - (a * b).sum() + 1e-5)
    oce = ((-d * torch.log(dd + 1e-5)) * mask).sum() / mask.sum()
    acc = ((dd.argmax(dim=3) == d.argmax(dim=3)).float() * mask[..., 0]).sum() / mask.sum()
    return torch.stack([iou(ys, gs), iou(hard, gs), seg / npix, oce, acc]).cpu().tolist()

  a, b = fused(), torch_ops()
  err = max(abs(x - y) / max(abs(x), 1e-12) for x, y in zip(a, b))
  ra, rb = alternate(fused, torch_ops, timed_host)
  C = nsc + no
  model = '   traffic model: (a) %.1f MB, (b) head %.1f MB + torch passes' % (npix * (C + nsc + no) * 4 / 1e6, npix * 2 * C * 4 / 1e6)
  return report('stats B=%d %dx%d nsc=%d no=%d' % (B, H, W, nsc, no), ra, rb, '   max rel. difference of the statistics (b is float32): %.2g%s' % (err, model))


def main():
  p = argparse.ArgumentParser()
  p.add_argument('--small', action='store_true', help='a rehearsal at toy sizes (numbers mean nothing)')
  args = p.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit('fg_eval_bench needs an MI355X; there is nothing to time without one')
  print('rounds %d, launches per round %d (median), warm-up %d' % (ROUNDS, REPS, WARM))
  ok = True
  for B in (1, 4):
    ok &= sweep(B, *((32, 64, 128, 256) if args.small else (256, 512, 1024, 2048)), 10)
  for B in (1, 4):
    for nsc in (9, 1):
      ok &= stats(B, *((32, 64) if args.small else (256, 512)), nsc, 8)
  print('condition (a) beats (b) beyond the spread of the rounds, everywhere: %s' % ok)


if __name__ == '__main__':
  main()
