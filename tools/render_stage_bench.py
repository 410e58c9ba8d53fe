#!/usr/bin/env python
"""Time of the render stage's two kernels on one MI355X: render_stage_bench.py [reps >= 21] [--out FILE].

Shapes: T = 20, 1024 x 2048 (d: 256 x 512 x 8) at B = 1 and 4, and T = 21, 530 x 500 (d: 133 x 125 x 8) at B = 1, on one-label
binary disc masks of a seeded scene.  Alternating in one process, per shape
  instance image   (a) ra_render_instances_u8, RA_RENDER_ADD and RA_RENDER_FIRST, against
                   (b) the reference's loop restated in torch calls: y.to(uint8), then per plane
                       total += u[:, t, ..., None] * colour[:, t] (FIRST: times (total == 0)), uint8 arithmetic that wraps, and
                   (b') for ADD only, one contraction: einsum('bthw,btk->bhwk') of floor(y) and the float colours (exact below
                       2^24), then & 255;
  orientation      (a) ra_render_orientation_u8 against
                   (b) ops.resize_linear on the eight channel planes, argmax, wheel[class] * mask, cast to uint8,
`rounds` times, each a median of `reps` calls between device events after a warm-up.  Printed: the median of the rounds and
their spread (min .. max), the bytes of the traffic model and the share of the 8 TB/s HBM peak that the model's bytes make of
the measured time, and whether (a) and (b) agree.  Traffic models, in bytes per image with P = H * W pixels:
  instances (a)   4 T P (y once) + 3 P (the image once)
  instances (b)   5 T P (the cast: float in, uint8 out) + 13 T P (per plane: u in, the [P,3] product out and in, total in and out)
  instances (b')  4 T P + 4 T P (floor) + 4 T P (the contraction reads it) + 12 P + 12 P + 24 P + 24 P + 3 P (float image, int64, & 255, cast)
  orientation (a) 4 Ps C (d once) + 4 P (mask) + 3 P
  orientation (b) 8 Ps C (channel planes) + 8 C P (the planes out and in) + 16 P (int64 classes out and in) + 12 P + 28 P + 15 P
                  (the gathered float colours out, in with the mask and out, in and out as uint8)
Last, the host time of utils/png.encode_colour8 for one 1024 x 2048 image of the instance kernel (level 6, median of 5)."""
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'rec-attend-public_amd'))
import numpy as np

from cityscapes_stage_bench import scene

HBM_BYTES_PER_S = 8.0e12


def main():
  import torch
  import analysis
  import ra_ops as ops
  from utils import png
  args = [a for a in sys.argv[1:] if not a.startswith('--')]
  reps = max(21, int(args[0])) if args else 31
  out_path = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else None
  if not torch.cuda.is_available():
    raise SystemExit('render_stage_bench.py needs an MI355X')
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

  def compare(B, forms):
    """forms: [(name, fn, model bytes)], the first one (a).  Alternating rounds; one line per form."""
    ts = [[] for _ in forms]
    for _ in range(rounds):
      for k, (_, fn, _) in enumerate(forms):
        ts[k].append(median_us(fn))
    meds = [float(np.median(t)) for t in ts]
    for (name, _, nbytes), t, med in zip(forms, ts, meds):
      say('%-3d %-44s %10.1f %18s %10.1f %12.1f' % (B, name, med, '%.1f..%.1f' % (min(t), max(t)), nbytes * 1e-6,
                                                   100 * nbytes / (med * 1e-6) / HBM_BYTES_PER_S))
    return meds

  wheel_f = torch.tensor(analysis.ORIENTATION_WHEEL, dtype=torch.float32, device=dev)
  sample = None
  for B, T, H, W, Hs, Ws in ((1, 20, 1024, 2048, 256, 512), (4, 20, 1024, 2048, 256, 512), (1, 21, 530, 500, 133, 125)):
    C, P, Ps = 8, H * W, Hs * Ws
    say('# B = %d, T = %d, %d x %d (d: %d x %d x %d); one-label disc masks; device events, %d rounds alternating, each a median of %d'
        % (B, T, H, W, Hs, Ws, C, rounds, reps))
    say('%-3s %-44s %10s %18s %10s %12s' % ('B', 'form', 'us', 'spread (min..max)', 'model MB', '% of 8 TB/s'))
    rng = np.random.RandomState(100 + B + T)
    y = scene(rng, B, T, H, W, dev)
    col = ops._render_table('instances', T, dev).unsqueeze(0).expand(B, T, 3).contiguous()
    col_f = col.to(torch.float32)

    def loop(first):
      def run():
        u = y.to(torch.uint8)
        total = torch.zeros((B, H, W, 3), dtype=torch.uint8, device=dev)
        for t in range(T):
          prod = u[:, t, :, :, None] * col[:, t, None, None, :]
          total += (total == 0).to(torch.uint8) * prod if first else prod
        return total
      return run

    def contraction():
      return (torch.einsum('bthw,btk->bhwk', torch.floor(y), col_f).to(torch.int64) & 255).to(torch.uint8)

    for first, mode in ((False, 'ADD'), (True, 'FIRST')):
      fused = lambda: ops.render_instances(y, colours=col, first=first)
      same = bool((fused() == loop(first)()).all())
      forms = [('(a) ra_render_instances_u8 %s' % mode, fused, B * (4.0 * T * P + 3 * P)),
               ('(b) torch, the reference\'s loop %s' % mode, loop(first), B * 18.0 * T * P)]
      if not first:
        same = same and bool((fused() == contraction()).all())
        forms.append(('(b\') torch, einsum + & 255', contraction, B * (12.0 * T * P + 75 * P)))
      meds = compare(B, forms)
      say('    %s: (a) / (b) = %.3f%s; (a) equals (b)%s: %s' % (mode, meds[0] / meds[1],
                                                           '' if first else ', (a) / (b\') = %.3f' % (meds[0] / meds[2]),
                                                           '' if first else ' and (b\')', same))
    if sample is None:
      sample = ops.render_instances(y)[0].cpu().numpy()

    lg = torch.tensor(rng.randn(B, Hs, Ws, C).astype(np.float32) * 2, device=dev)
    d = torch.softmax(lg, dim=-1).contiguous()
    mask = (y.sum(dim=1) > 0).to(torch.float32).contiguous()
    fused = lambda: ops.render_orientation(d, mask)

    def composed():
      full = ops.resize_linear(d.permute(0, 3, 1, 2).contiguous(), H, W)
      return (wheel_f[full.argmax(dim=1)] * mask[..., None]).to(torch.uint8)

    differ = int((fused() != composed()).any(dim=-1).sum())
    meds = compare(B, [('(a) ra_render_orientation_u8', fused, B * (4.0 * Ps * C + 7 * P)),
                       ('(b) resize_linear x 8 + argmax + gather', composed, B * (8.0 * Ps * C + 8.0 * C * P + 71 * P))])
    say('    orientation: (a) / (b) = %.3f; pixels where (a) and (b) differ: %d of %d (the resize of (b) keeps its coordinate in '
        'float); mask: %.1f %% of the pixels' % (meds[0] / meds[1], differ, B * P, 100 * float(mask.mean())))
    del y, mask

  ts = []
  for _ in range(5):
    t0 = time.perf_counter()
    data = png.encode_colour8(sample)
    ts.append(time.perf_counter() - t0)
  say('# utils/png.encode_colour8, one %d x %d instance image, level 6, host: median of 5 %.1f ms (%.1f..%.1f), %d bytes'
      % (sample.shape[0], sample.shape[1], 1e3 * float(np.median(ts)), 1e3 * min(ts), 1e3 * max(ts), len(data)))
  if out_path:
    with open(out_path, 'w') as f:
      f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
  main()
