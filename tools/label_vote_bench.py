#!/usr/bin/env python
"""Time of the Cityscapes output stage behind a label-image segmentation on one MI355X: label_vote_bench.py [reps >= 21] [--out FILE].

At B = 1 and 4, T = 20, 1024 x 2048, the ten default thresholds (0.0 ... 0.9), remove_tiny = 400, on the soft masks of a seeded
scene (overlapping discs) and a label image of blocks of thing and stuff labels, alternating in one process
  (a1) the sweep alone, ops.label_vote_sweep: class, score and size of every instance at every threshold from one read of y,
  (a2) the sweep + ten ops.label_planes: also every threshold's binary planes, and
  (b)  what the ops without them offer for the same input: the per-threshold chain of cityscapes_eval.iter_label_instances
       behind apply_one_label on a full-size one-hot map [B,1024,2048,9] — apply_threshold, mask_foreground, remove_tiny
       (pair_stats + the kernel), the resampling vote,
`rounds` times, each a median of `reps` launches between device events after a warm-up.  Printed per batch size: the median of
the rounds and their spread (min .. max), the bytes of the traffic model and the share of the 8 TB/s HBM peak that the
model's bytes make of the measured time, and whether (a) and (b) name every instance alike.  Traffic model: (a1) y once + the
label image; a label_planes call reads y and writes the planes; (b) per threshold: apply_threshold reads and writes a
[B,T,H,W], mask_foreground reads and writes one, pair_stats reads one, remove_tiny's clone reads and writes one, the vote reads
one (+ the one-hot map): eight passes, plus apply_one_label's three once."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'rec-attend-public_amd'))
import numpy as np

HBM_BYTES_PER_S = 8.0e12
THING = (24, 25, 26, 27, 28, 31, 32, 33)


def scene(rng, B, T, H, W, dev):
  """Soft overlapping disc masks [B,T,H,W] in [0, 1] (exact zeros away from the discs) and a label image of 64 x 128 blocks."""
  import torch
  yy = torch.arange(H, device=dev, dtype=torch.float32)[:, None]
  xx = torch.arange(W, device=dev, dtype=torch.float32)[None, :]
  y = torch.zeros((B, T, H, W), device=dev)
  for b in range(B):
    for t in range(T):
      r = rng.uniform(0.05, 0.2) * H
      cy, cx = rng.uniform(0, H), rng.uniform(0, W)
      y[b, t] = torch.clamp(1.5 * (1 - torch.sqrt((yy - cy) ** 2 + (xx - cx) ** 2) / r), 0, 1) * float(rng.uniform(0.6, 1.0))
  pool = np.array(THING + (7, 8, 11, 21, 23, 0), np.uint8)
  blocks = pool[rng.randint(0, len(pool), (B, H // 64, W // 128))]
  labels = torch.from_numpy(np.repeat(np.repeat(blocks, 64, axis=1), 128, axis=2)).to(dev)
  return y.contiguous(), labels.contiguous()


def main():
  import torch
  import ra_ops as ops
  from utils import postprocess as pp
  args = [a for a in sys.argv[1:] if not a.startswith('--')]
  reps = max(21, int(args[0])) if args else 21
  out_path = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else None
  if not torch.cuda.is_available():
    raise SystemExit('label_vote_bench.py needs an MI355X')
  dev = torch.device('cuda:0')
  rounds, lines = 5, []

  def say(s):
    print(s, flush=True)
    lines.append(s)

  def median_us(fn):
    for _ in range(3):
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

  T, H, W, remove_tiny = 20, 1024, 2048, 400
  ths = [i * 0.1 for i in range(10)]
  lut = ops.label_class_lut('labelIds')
  lut_dev = torch.from_numpy(lut).to(dev)
  say('# label-image vote, T = %d, %d x %d, %d thresholds, remove_tiny = %d; soft disc masks; device events, %d rounds alternating '
      '(a1), (a2), (b), each a median of %d' % (T, H, W, len(ths), remove_tiny, rounds, reps))
  say('%-3s %-44s %10s %20s %10s %12s' % ('B', 'form', 'us', 'spread (min..max)', 'model MB', '% of 8 TB/s'))
  for B in (1, 4):
    rng = np.random.RandomState(200 + B)
    y, labels = scene(rng, B, T, H, W, dev)
    conf = torch.from_numpy(rng.uniform(0.55, 1.0, (B, T)).astype(np.float32)).to(dev)
    cls = lut_dev[labels.long()]
    sem = torch.nn.functional.one_hot(cls.long(), 9).to(torch.float32).contiguous()   # [B,H,W,9]: (b)'s input, not timed
    fg = (cls > 0).to(torch.float32)

    def sweep():
      return ops.label_vote_sweep(y, labels, lut, ths, conf, remove_tiny)

    def sweep_planes():
      sw = ops.label_vote_sweep(y, labels, lut, ths, conf, remove_tiny)
      for k, th in enumerate(ths):
        ops.label_planes(y, labels, lut, th, keep=sw['keep'][k])
      return sw

    def chain():
      one = pp.apply_one_label(y)
      c, labs = conf.clone(), []
      for th in ths:
        y_bin = pp.mask_foreground(pp.apply_threshold(one, th), fg)
        y_bin, c = pp.remove_tiny(y_bin, c, threshold=remove_tiny)
        labs.append(ops.instance_class_vote(y_bin, sem, c)[2])
      return torch.stack(labs)

    same = bool(torch.equal(sweep()['label_id'], chain()))
    t1, t2, tb = [], [], []
    for _ in range(rounds):
      t1.append(median_us(sweep))
      t2.append(median_us(sweep_planes))
      tb.append(median_us(chain))
    plane = 4.0 * B * T * H * W
    bytes_1 = plane + B * H * W
    bytes_2 = bytes_1 + len(ths) * (2 * plane + B * H * W)
    bytes_b = 3 * plane + len(ths) * (8 * plane + 4.0 * B * H * W * 10)
    for name, ts, nbytes in (('(a1) sweep', t1, bytes_1), ('(a2) sweep + 10 label_planes', t2, bytes_2),
                             ('(b) per-threshold chain on the one-hot map', tb, bytes_b)):
      med = float(np.median(ts))
      say('%-3d %-44s %10.1f %20s %10.1f %12.1f' % (B, name, med, '%.1f..%.1f' % (min(ts), max(ts)), nbytes * 1e-6,
                                                   100 * nbytes / (med * 1e-6) / HBM_BYTES_PER_S))
    say('    (a1) / (b) = %.4f, (a2) / (b) = %.3f; label_id of (a) and (b) identical at every threshold: %s; thing pixels: %.1f %%' % (
        float(np.median(t1)) / float(np.median(tb)), float(np.median(t2)) / float(np.median(tb)), same, 100 * float(fg.mean())))
    del y, labels, sem, fg, cls
  if out_path:
    with open(out_path, 'w') as f:
      f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
  main()
