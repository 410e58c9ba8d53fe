#!/usr/bin/env python
"""Time of the Cityscapes output stage's class vote on one MI355X: cityscapes_stage_bench.py [reps >= 21] [--out FILE].

At B = 1 and 4, T = 20, 1024 x 2048 labels from a 256 x 512 semantic map with C = 9, on the one-label binary masks of a
seeded scene (discs), alternating in one process
  (a) the fused vote, ra_instance_class_vote_f32 (the resize of the semantic map evaluated inside the reduction), and
  (b) the composition the ops without it offer: ops.resize_linear on the nine channel planes, then
      torch.einsum('bthw,bchw->btc') / (H * W),
`rounds` times, each a median of `reps` launches between device events after a warm-up.  Printed per batch size: the median
of the rounds and their spread (min .. max) for both, the bytes of the traffic model (y once + the semantic map once for (a);
(b) also writes and re-reads the C full-size planes) and the share of the 8 TB/s HBM peak that the model's bytes make of
the measured time, and the largest difference between the two results."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'rec-attend-public_amd'))
import numpy as np

HBM_BYTES_PER_S = 8.0e12


def scene(rng, B, T, H, W, dev):
  """One-label binary disc masks [B,T,H,W], built on the device (no pixel belongs to two instances)."""
  import torch
  yy = torch.arange(H, device=dev, dtype=torch.float32)[:, None]
  xx = torch.arange(W, device=dev, dtype=torch.float32)[None, :]
  y = torch.zeros((B, T, H, W), device=dev)
  for b in range(B):
    for t in range(T):
      r = rng.uniform(0.05, 0.2) * H
      cy, cx = rng.uniform(0, H), rng.uniform(0, W)
      y[b, t] = torch.clamp(1.5 * (1 - torch.sqrt((yy - cy) ** 2 + (xx - cx) ** 2) / r), 0, 1)
  am = y.argmax(dim=1, keepdim=True)
  return ((torch.arange(T, device=dev)[None, :, None, None] == am) & (y > 0.3)).to(torch.float32).contiguous()


def main():
  import torch
  import ra_ops as ops
  args = [a for a in sys.argv[1:] if not a.startswith('--')]
  reps = max(21, int(args[0])) if args else 31
  out_path = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else None
  if not torch.cuda.is_available():
    raise SystemExit('cityscapes_stage_bench.py needs an MI355X')
  dev = torch.device('cuda:0')
  rounds, lines = 5, []

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

  T, H, W, Hs, Ws, C = 20, 1024, 2048, 256, 512, 9
  say('# class vote, T = %d, %d x %d <- %d x %d, C = %d; one-label disc masks; device events, %d rounds alternating (a) and (b), each a '
      'median of %d' % (T, H, W, Hs, Ws, C, rounds, reps))
  say('%-3s %-36s %10s %18s %10s %12s' % ('B', 'form', 'us', 'spread (min..max)', 'model MB', '% of 8 TB/s'))
  for B in (1, 4):
    rng = np.random.RandomState(100 + B)
    y = scene(rng, B, T, H, W, dev)
    lg = torch.tensor(rng.randn(B, Hs, Ws, C).astype(np.float32) * 2, device=dev)
    sem = torch.floor(torch.softmax(lg, dim=-1) * 255) / 255  # the 8-bit round trip of the pre-stage
    sem = sem.contiguous()
    planes = sem.permute(0, 3, 1, 2).contiguous()              # [B,C,Hs,Ws] for (b): not timed

    def fused():
      return ops.instance_class_vote(y, sem)

    def composed():
      return torch.einsum('bthw,bchw->btc', y, ops.resize_linear(planes, H, W)) / float(H * W)

    diff = float((fused() - composed()).abs().max())
    ta, tb = [], []
    for _ in range(rounds):
      ta.append(median_us(fused))
      tb.append(median_us(composed))
    bytes_a = 4.0 * B * (T * H * W + Hs * Ws * C)
    bytes_b = bytes_a + 2 * 4.0 * B * C * H * W
    for name, ts, nbytes in (('(a) fused vote', ta, bytes_a), ('(b) resize_linear x 9 + einsum', tb, bytes_b)):
      med = float(np.median(ts))
      say('%-3d %-36s %10.1f %18s %10.1f %12.1f' % (B, name, med, '%.1f..%.1f' % (min(ts), max(ts)), nbytes * 1e-6,
                                                   100 * nbytes / (med * 1e-6) / HBM_BYTES_PER_S))
    say('    (a) / (b) = %.3f; max |vote (a) - vote (b)| = %.3g; foreground of the masks: %.1f %% of the pixels' % (
        float(np.median(ta)) / float(np.median(tb)), diff, 100 * float(y.sum(dim=1).mean())))
    del y, planes
  if out_path:
    with open(out_path, 'w') as f:
      f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
  main()
