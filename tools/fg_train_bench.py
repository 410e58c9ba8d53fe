#!/usr/bin/env python
"""First measurements of fg_model training (profiles/fg_train.txt): nobody has measured these before, there is no bar.

parity  the loss-gradient kernel (ra_fg_loss_bwd_f32) against float64 autograd for every case of
        tests/test_fg_train_gpu.py, beside the same formulas evaluated in float32 torch on the CPU: max |error| / max |reference|.
kernel  its time at 256 x 512, B = 4 for the channel counts of the run scripts (1, 9, 11, 17) and both losses, and the
        achieved bytes / s of its traffic model — 2 (nsc + no) floats read and nsc + no written per pixel — against 8 TB/s.
step    the time of one FgTrainStep.run (augmentation, forward, backward, optimizer) for the reduced net of tests/fg_oracle.py
        and for the command line's default net (fg_model_train.py:425-437 of the reference: ten cnn and eleven dcnn layers of 8
        to 128 channels, with its skips) with 1 + 8 classes at the KITTI size 128 x 448, its second dcnn layer at 64 instead of
        128 channels so that no layer's input (previous map + skip) exceeds 128: the largest run-script-shaped net that trains.

A figure is the median over ROUNDS rounds of the median of REPS repetitions timed between device events after a warm-up; the
spread of the rounds is printed beside it."""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(HERE, '..', 'rec-attend-public_amd'), os.path.join(HERE, '..', 'oracle'), os.path.join(HERE, '..', 'tests')]
import fg_model  # noqa: E402
import fg_oracle as fo  # noqa: E402
import ra_fg_train  # noqa: E402
import ra_ops as ops  # noqa: E402

ROUNDS, REPS, WARM = 5, 21, 5
HBM_PEAK = 8e12  # bytes / s


def timed(fn, reps=REPS, warm=WARM):
  rounds = []
  for _ in range(ROUNDS):
    ts = []
    for i in range(warm + reps):
      a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      a.record()
      fn()
      b.record()
      b.synchronize()
      if i >= warm:
        ts.append(a.elapsed_time(b) * 1e3)
    rounds.append(float(np.median(ts)))
  return float(np.median(rounds)), min(rounds), max(rounds)


def parity(emit):
  import test_fg_train_gpu as tg
  emit('parity: max |error| / max |reference| against float64 autograd (tests/fg_train_oracle.py)')
  emit('  nsc no loss  npix   kernel      float32 torch   bound (min(4 x float32 torch, worst float32 torch of the table))')
  for case, (z, y, d, ref, e32) in tg.head_table().items():
    nsc, no, seg, npix = case
    dz, _ = tg.run_head(z, y, d, nsc, no, seg)
    err = tg._rel_err(dz.cpu().numpy().astype(np.float64), ref)
    emit('  %3d %2d %-4s %5d   %.3e   %.3e       %.3e' % (nsc, no, seg, npix, err, e32, tg.head_bound(case)))


def kernel(emit, B, H, W):
  emit('kernel: ra_fg_loss_bwd_f32 at B = %d, %d x %d' % (B, H, W))
  rng = np.random.RandomState(0)
  npix = B * H * W
  for nsc, no in ((1, 0), (1, 8), (3, 8), (9, 8)):
    C = nsc + no
    z = torch.from_numpy((rng.randn(npix, C) * 3).astype(np.float32)).cuda()
    y = torch.from_numpy((rng.rand(npix, 1) < 0.3).astype(np.float32) if nsc == 1 else
                         np.eye(nsc, dtype=np.float32)[np.where(rng.rand(npix) < 0.3, rng.randint(1, nsc, npix), 0)]).cuda()
    d = torch.from_numpy(np.eye(8, dtype=np.float32)[rng.randint(0, 8, npix)]).cuda() if no else None
    sums = ops.fg_stat_sums(z, y, d, nsc, no)
    status = torch.zeros(1, dtype=torch.int32, device='cuda')
    for seg in ('iou', 'bce'):
      med, lo, hi = timed(lambda: ops.fg_loss_backward(z, y, d, nsc, no, seg, sums, status=status))
      nbytes = 3 * C * 4 * npix
      emit('  C = %2d (nsc %d + no %d) %-4s %7.1f us [%.1f .. %.1f]   %6.1f MB   %.2f TB/s = %.0f %% of 8 TB/s' % (
          C, nsc, no, seg, med, lo, hi, nbytes / 1e6, nbytes / med / 1e6, 100 * nbytes / (med * 1e-6) / HBM_PEAK))


def step(emit, name, opt, B, H, W):
  nsc = int(opt.get('num_semantic_classes', 1))
  model = fg_model.get_model(opt)
  ts = ra_fg_train.FgTrainStep(model)
  rng = np.random.RandomState(1)
  x = torch.from_numpy(rng.rand(B, H, W, 3).astype(np.float32)).cuda()
  y = torch.from_numpy((rng.rand(B, H, W) < 0.3).astype(np.float32) if nsc == 1 else
                       np.eye(nsc, dtype=np.float32)[np.where(rng.rand(B, H, W) < 0.3, rng.randint(1, nsc, (B, H, W)), 0)]).cuda()
  d = torch.from_numpy(np.eye(8, dtype=np.float32)[rng.randint(0, 8, (B, H, W))]).cuda() if opt.get('add_orientation') else None
  med, lo, hi = timed(lambda: ts.run(x, y, d), reps=9, warm=3)
  ts.flush_status()
  nparam = sum(model[k].numel() for k in ts.bucket.names)
  emit('  %-44s B = %d, %d x %d, %s: %9.1f us per step [%.1f .. %.1f]   (%d layers, %d parameters)' % (
      name, B, H, W, opt['optimizer'], med, lo, hi, len(opt['cnn_depth']) + len(opt['dcnn_depth']), nparam))


def default_net(optimizer):
  import fg_model_train
  args = fg_model_train.build_parser().parse_args(['--dataset', 'kitti', '--add_skip_conn', '--add_orientation', '--dcnn_depth',
                                                   '128,64,64,64,32,32,16,16,8,8,9', '--segm_loss_fn', 'bce', '--optimizer', optimizer])
  return fg_model_train.make_opt(args)


def main():
  p = argparse.ArgumentParser()
  p.add_argument('--small', action='store_true', help='a rehearsal at toy sizes (numbers mean nothing)')
  p.add_argument('--out', default=os.path.join(HERE, '..', 'profiles', 'fg_train.txt'))
  args = p.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit('fg_train_bench needs an MI355X; there is nothing to time without one')
  lines = []

  def emit(line):
    print(line, flush=True)
    lines.append(line)

  emit('python tools/fg_train_bench.py%s — rounds %d, repetitions per round %d (median; steps: 9), warm-up %d (steps: 3)' % (
      ' --small' if args.small else '', ROUNDS, REPS, WARM))
  parity(emit)
  kernel(emit, *((1, 32, 64) if args.small else (4, 256, 512)))
  emit('step: one FgTrainStep.run, eager stream launches')
  for optimizer in ('adam', 'momentum'):
    red = dict(fo.reduced_opt(nsc=1, orientation=True), padding=2, segm_loss_fn='bce', optimizer=optimizer)
    step(emit, 'reduced net (tests/fg_oracle.reduced_opt)', red, 2, 16, 24)
    step(emit, 'default net (dcnn layer 1 at 64), 1 + 8 classes', default_net(optimizer), *((1, 32, 64) if args.small else (8, 128, 448)))
  with open(args.out, 'w') as f:
    f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
  main()
