#!/usr/bin/env python
"""Times a KITTI-shaped batch of MIXED full sizes through the ragged entry points against the same images through the uniform
entry points, one call per size group — what the kernels could do before the ragged forms existed (profiles/mixed_sizes.txt).

B = 8 images drawn from 370 x 1224, 374 x 1238, 375 x 1242 and 376 x 1241 in mixed order; KITTI's network size 128 x 448 and
T = 20 (cmd_args_parser.INP_DIM); K = 1 and K = 10 thresholds; the instance evaluator with a foreground and the dilation, and
the pre-stage's sweep.
  (1) one ragged call over the batch;
  (2) the uniform entry point once per size group, on tensors gathered BEFORE the clock starts (the host-side split and the
      scatter of the results back into batch order are not charged): the sum of the group times is reported;
  (3) eight images of ONE size (375 x 1242) through both entries: what the table costs the uniform case.
The routes alternate for ROUNDS rounds; a round is the median of REPS calls timed one by one between device events after a
warm-up.  Reported: the median of the rounds and their spread.  The counts of (1) and (2) are compared image by image."""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(HERE, '..', 'rec-attend-public_amd'), os.path.join(HERE, '..', 'oracle'), os.path.join(HERE, '..', 'tests')]
import cmd_args_parser as cap  # noqa: E402
import ra_ops as ops  # noqa: E402

ROUNDS, REPS, WARM = 5, 11, 3
KITTI_SIZES = ((370, 1224), (374, 1238), (375, 1242), (376, 1241))
ORDER = (2, 0, 2, 3, 1, 2, 0, 3)  # indices into KITTI_SIZES: a batch in dataset order mixes the sizes


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


def images(sizes, T, seed):
  """Per image: ids int32 [h,w] (T + 2 discs), fg uint8 0 / 1, sweep labels uint8."""
  import fg_eval_oracle as feo
  rng = np.random.RandomState(seed)
  ids, fg, gt = [], [], []
  for h, w in sizes:
    rr, cc = np.mgrid[0:h, 0:w].astype(np.float32)
    img = np.zeros((h, w), np.int32)
    for i in range(T + 2):
      cy, cx, rad = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(0.05, 0.2) * min(h, w)
      img[(rr - cy) ** 2 + (cc - cx) ** 2 <= rad ** 2] = i + 1
    ids.append(img)
    lab = feo.disc_labels(rng, 1, h, w, n_disc=12)[0]
    gt.append(lab)
    fg.append((lab > 0).astype(np.uint8))
  return ids, fg, gt


def report(what, rounds):
  return '%s %8.1f us [%.1f .. %.1f]' % (what, np.median(rounds), min(rounds), max(rounds))


def case(sizes, T, Hs, Ws, K, tag):
  import fg_eval_oracle as feo
  B = len(sizes)
  rng = np.random.RandomState(7)
  yc = torch.from_numpy(feo.smooth_map(rng, B * T, Hs, Ws).reshape(B, T, Hs, Ws) * rng.uniform(0.3, 1.0, (B, T, 1, 1)).astype(np.float32)).cuda()
  src = torch.from_numpy(feo.smooth_map(rng, B, Hs, Ws)).cuda()
  inst_id = torch.from_numpy(np.tile(np.arange(1, T + 1, dtype=np.int32), (B, 1))).cuda()
  ids, fg, gt = images(sizes, T, 11)
  thr = [0.3] if K == 1 else [0.1 * k for k in range(K)]
  ids_flat, geo = ops.pack_ragged(ids, torch.int32)
  fg_flat, _ = ops.pack_ragged(fg, torch.uint8)
  gt_flat, _ = ops.pack_ragged(gt, torch.uint8)
  groups = {}
  for b, s in enumerate(sizes):
    groups.setdefault(tuple(s), []).append(b)
  dev = lambda arrs: torch.from_numpy(np.stack(arrs)).cuda()
  per_group = [(m, yc[m].contiguous(), src[m].contiguous(), inst_id[m].contiguous(), dev([ids[b] for b in m]), dev([fg[b] for b in m]),
                dev([gt[b] for b in m])) for m in groups.values()]

  ragged_eval = lambda: ops.instance_eval_counts_ragged(yc, ids_flat, geo, inst_id, thr, fg_flat=fg_flat, morph=True, check_fg=False)
  ragged_sweep = lambda: ops.fg_sweep_counts_ragged_device(src, gt_flat, geo, thr)
  group_eval = [(lambda g=g: ops.instance_eval_counts(g[1], g[4], g[3], thr, fg=g[5], morph=True, check_fg=False)) for g in per_group]
  group_sweep = [(lambda g=g: ops.fg_sweep_counts_device(g[2], g[6], thr)) for g in per_group]
  # the same integers, image by image
  inter, area = ragged_eval()
  counts = ragged_sweep()
  same = True
  for g, fe, fs in zip(per_group, group_eval, group_sweep):
    gi, ga = fe()
    same &= bool(torch.equal(gi, inter[g[0]]) and torch.equal(ga, area[g[0]]) and torch.equal(fs(), counts[g[0]]))
  r = {k: [] for k in ('eval_ragged', 'eval_groups', 'sweep_ragged', 'sweep_groups')}
  for _ in range(ROUNDS):
    r['eval_ragged'].append(timed_events(ragged_eval))
    r['eval_groups'].append(sum(timed_events(f) for f in group_eval))
    r['sweep_ragged'].append(timed_events(ragged_sweep))
    r['sweep_groups'].append(sum(timed_events(f) for f in group_sweep))
  print('%s B=%d (%d size groups) T=%d %dx%d K=%-2d ragged == per-group counts: %s' % (tag, B, len(groups), T, Hs, Ws, K, same))
  print('   instance evaluator, fg + morph: %s   %s   groups / ragged x%.2f' % (
      report('(1) one ragged call', r['eval_ragged']), report('(2) sum over %d uniform calls' % len(groups), r['eval_groups']),
      np.median(r['eval_groups']) / np.median(r['eval_ragged'])))
  print('   sweep:                          %s   %s   groups / ragged x%.2f' % (
      report('(1) one ragged call', r['sweep_ragged']), report('(2) sum over %d uniform calls' % len(groups), r['sweep_groups']),
      np.median(r['sweep_groups']) / np.median(r['sweep_ragged'])), flush=True)


def main():
  p = argparse.ArgumentParser()
  p.add_argument('--small', action='store_true', help='a rehearsal at toy sizes (numbers mean nothing)')
  args = p.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit('mixed_sizes_bench needs an MI355X; there is nothing to time without one')
  Hs, Ws, T = cap.INP_DIM['kitti']
  table = KITTI_SIZES
  if args.small:
    Hs, Ws, T, table = 16, 56, 4, ((37, 122), (37, 124), (38, 124), (38, 123))
  print('rounds %d, calls per round %d (median), warm-up %d; times: median of the rounds [fastest .. slowest round]' % (ROUNDS, REPS, WARM))
  mixed = [table[i] for i in ORDER]
  for K in (1, 10):
    case(mixed, T, Hs, Ws, K, 'mixed  ')
    case([table[2]] * len(ORDER), T, Hs, Ws, K, 'uniform')  # (3): one group, so (2) is the uniform entry on the whole batch


if __name__ == '__main__':
  main()
