#!/usr/bin/env python
"""Time of the matching step of the Cityscapes instance-level AP on one MI355X: cityscapes_ap_bench.py [reps >= 21] [--out FILE].

At B = 1 and 4, T = 20, 1024 x 2048, on the one-label binary masks of a seeded scene (discs) and a generated instance-id image
with about 60 instances (discs of other centres on a ground of a few label ids), alternating in one process
  (a) ops.gt_instance_catalog + ops.instance_overlap (ra_gt_instance_catalog_i32, ra_instance_overlap_f32), and
  (b) what the ops without them offer for the same counts: the ground truth expanded to [B,G,H,W] float masks and
      ops.pair_stats(y, gt_masks) over chunks of 32 entries (its limit), with the expansion's own time reported apart,
`rounds` times, each a median of `reps` launches between device events after a warm-up.  The counts of (a) and (b) are
compared for equality.  Printed per batch size: the median of the rounds and their spread (min .. max), the bytes of the
traffic model — y once + gt_ids twice (catalogue and overlap) for (a); for (b) y once per chunk + the G float masks written and
read — and the share of the 8 TB/s HBM peak that the model's bytes make of the measured time."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'rec-attend-public_amd'))
import numpy as np

from cityscapes_stage_bench import scene

HBM_BYTES_PER_S = 8.0e12
PAIR_CHUNK = 32  # ra_pair_stats_f32: M <= 32


def gt_scene(rng, B, H, W, n_inst, dev):
  """int32 [B,H,W]: label ids 23 / 7 / 1 as ground, n_inst discs labelId * 1000 + k on top (later ones cover earlier ones)."""
  import torch
  yy = torch.arange(H, device=dev, dtype=torch.float32)[:, None]
  xx = torch.arange(W, device=dev, dtype=torch.float32)[None, :]
  gt = torch.full((B, H, W), 7, dtype=torch.int32, device=dev)
  gt[:, :H // 3] = 23
  gt[:, H - H // 16:] = 1
  for b in range(B):
    for k in range(n_inst):
      r = rng.uniform(0.02, 0.12) * H
      cy, cx = rng.uniform(0.3 * H, 0.95 * H), rng.uniform(0, W)
      gt[b][(yy - cy) ** 2 + (xx - cx) ** 2 < r * r] = int(rng.choice([24, 25, 26, 27, 28, 33])) * 1000 + k
  return gt.contiguous()


def main():
  import torch
  import ra_ops as ops
  args = [a for a in sys.argv[1:] if not a.startswith('--')]
  reps = max(21, int(args[0])) if args else 21
  out_path = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else None
  if not torch.cuda.is_available():
    raise SystemExit('cityscapes_ap_bench.py needs an MI355X')
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

  T, H, W = 20, 1024, 2048
  say('# AP matching step, T = %d, %d x %d; one-label disc masks, about 60 ground-truth instances; device events, %d rounds '
      'alternating (a) and (b), each a median of %d' % (T, H, W, rounds, reps))
  say('%-3s %-44s %10s %20s %10s %12s' % ('B', 'form', 'us', 'spread (min..max)', 'model MB', '% of 8 TB/s'))
  for B in (1, 4):
    rng = np.random.RandomState(200 + B)
    y = scene(rng, B, T, H, W, dev)
    gt = gt_scene(rng, B, H, W, 60, dev)

    def ours():
      cat = ops.gt_instance_catalog(gt, check_status=False)
      return cat, ops.instance_overlap(y, gt, cat)

    (ids, pixels, count, status), (inter, pred) = ours()
    assert int(status.abs().max()) == 0
    G = int(count.max())
    ids_g = ids[:, :G].contiguous()  # -1 beyond an image's count: matches no pixel

    def expand():
      return (gt[:, None] == ids_g[:, :, None, None]).to(torch.float32)

    def parent():
      masks = expand()
      return torch.cat([ops.pair_stats(y, masks[:, g0:g0 + PAIR_CHUNK].contiguous(), want=('inter',))['inter']
                        for g0 in range(0, G, PAIR_CHUNK)], dim=2)

    ref = parent()
    equal = bool(torch.equal(ref.to(torch.int32), inter[:, :, :G])) and bool(torch.equal(inter.sum(dim=2), pred))
    ta, tb, te = [], [], []
    for _ in range(rounds):
      ta.append(median_us(ours))
      tb.append(median_us(parent))
      te.append(median_us(expand))
    chunks = (G + PAIR_CHUNK - 1) // PAIR_CHUNK
    bytes_a = 4.0 * B * H * W * (T + 2)
    bytes_b = 4.0 * B * H * W * (chunks * T + 1 + 2 * G)
    for name, ts, nbytes in (('(a) catalogue + overlap', ta, bytes_a),
                             ('(b) expansion + pair_stats x %d' % chunks, tb, bytes_b),
                             ('    the expansion of (b) alone', te, 4.0 * B * H * W * (1 + G))):
      med = float(np.median(ts))
      say('%-3d %-44s %10.1f %20s %10.1f %12.1f' % (B, name, med, '%.1f..%.1f' % (min(ts), max(ts)), nbytes * 1e-6,
                                                   100 * nbytes / (med * 1e-6) / HBM_BYTES_PER_S))
    say('    (a) / (b) = %.3f; counts equal: %s; G = %d catalogue entries (per image: %s); foreground of the masks: %.1f %% of the pixels'
        % (float(np.median(ta)) / float(np.median(tb)), equal, G, count.tolist(), 100 * float(y.sum(dim=1).mean())))
    del y, gt, ref
  if out_path:
    with open(out_path, 'w') as f:
      f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
  main()
