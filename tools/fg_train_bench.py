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

--wide writes profiles/fg_train_wide.txt instead, the first measurement of the opt-in wide path (FgTrainStep(model, wide=True)):
parity  the wide filter-gradient kernel against _wgrad_ref in float64 for the cases of tests/test_wgrad_wide_gpu.py, beside float32 torch.
layers  every layer of more than 128 output channels of the nets run_kitti.sh (128 x 448) and run_cityscapes.sh (256 x 512) train,
        at the run scripts' batch size 8: ra_conv3x3_wide_f32 (forward) against ra_conv3x3_wgrad_wide_acc_f32 on the same layer — the
        algorithmic FLOPs 2 * 9 * Cin * Cout * B * H * W are the same — as a ratio and as a share of the f32 MFMA's 157.3 TF/s, with
        the K split and the workspace the chooser picks.
step    one FgTrainStep(model, wide=True).run of both nets at those sizes, eager stream launches, synthetic data.

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


def step(emit, name, opt, B, H, W, wide=False):
  nsc = int(opt.get('num_semantic_classes', 1))
  model = fg_model.get_model(opt)
  ts = ra_fg_train.FgTrainStep(model, wide=wide)
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


F32_MFMA_PEAK = 157.3e12  # FLOP / s, v_mfma_f32_16x16x4_f32 on 256 CUs


def wide_parity(emit):
  import test_wgrad_wide_gpu as tw
  from wgrad_form_cases import F32_BAR, _rel
  emit('parity: ra_conv3x3_wgrad_wide_acc_f32, max |error| / max |reference| against _wgrad_ref in float64; bar %g' % F32_BAR)
  emit('   Cin Cout  B   Hs x Ws ups  split x tiles    dW kernel   dW float32 torch   db kernel   db float32 torch')
  for case in tw.CASES:
    cin, cout, B, Hs, Ws, ups = case
    x, du, dw, db, e32w, e32b = tw.reference(*case)
    gw, gb = tw.run(x, du, torch.zeros(3, 3, cin, cout), torch.zeros(cout), ups=ups)
    plan = ops.wgrad_wide_plan(*case)
    emit('  %4d %4d  %d  %3d x %-3d  %d     %2d x %-3d      %.3e   %.3e          %.3e   %.3e' % (
        cin, cout, B, Hs, Ws, ups, plan['split'], plan['tiles_per_part'], _rel(gw, dw), e32w, _rel(gb, db), e32b))


def wide_layers(emit, name, opt, B, H, W):
  """Forward and filter gradient of every layer of more than 128 output channels, at the map sizes of an H x W input."""
  d = fg_model.derive(opt)
  emit('layers of %s at B = %d, %d x %d: forward = ra_conv3x3_wide_f32 (scale 1, shift b, no ReLU, no pool), filter gradient = '
       'ra_conv3x3_wgrad_wide_acc_f32 once per source' % (name, B, H, W))
  emit('  layer      Cin (sources)  Cout  x map      ups  GFLOP   forward us  TF/s   wgrad us [min .. max]     TF/s  % of 157.3    ratio   split x tiles  workspace MB')
  rng = np.random.RandomState(2)
  dev = torch.device('cuda')
  worst_ws, tot_f, tot_g = 0, 0.0, 0.0
  down = [1]
  for p in d['cnn_pool']:
    down.append(down[-1] * p)
  cur = down[-1]
  layers = [('cnn', i, [d['cnn_channels'][i]], d['cnn_channels'][i + 1], down[i], 0) for i in range(len(d['cnn_pool']))]
  for i in range(len(d['dcnn_pool'])):
    layers.append(('dcnn', i, ra_fg_train._layer_sources(d, 'dcnn', i), d['dcnn_channels'][i + 1], cur, int(d['dcnn_pool'][i] == 2)))
    cur //= d['dcnn_pool'][i]
  for scope, i, sources, cout, dn, ups in layers:
    if cout <= 128:
      continue
    Hs, Ws = H // dn, W // dn
    up = 1 + ups
    xs = [torch.from_numpy(rng.randn(B, Hs, Ws, c).astype(np.float32)).to(dev) for c in sources]
    cin = sum(sources)
    tr = scope == 'dcnn'
    w = torch.from_numpy((rng.randn(*((3, 3, cout, cin) if tr else (3, 3, cin, cout))) * np.sqrt(2.0 / (9 * cin))).astype(np.float32)).to(dev)
    b = torch.zeros(cout, device=dev)
    ones = torch.ones(cout, device=dev)
    wp = ops.pack_wide_weights_dev(w, transposed=tr)
    u = torch.empty((B, Hs * up, Ws * up, cout), device=dev)
    du = torch.from_numpy(rng.randn(B, Hs * up, Ws * up, cout).astype(np.float32)).to(dev)
    gw, gb = torch.zeros_like(w), torch.zeros(cout, device=dev)
    fwd = lambda: ops.conv_wide(xs[0], wp, ones, b, cout, relu=False, pool=1, src1=xs[1] if len(xs) > 1 else None, upsample=bool(ups), out=u)
    plans = [ops.wgrad_wide_plan(c, cout, B, Hs, Ws, ups) for c in sources]
    ws = torch.empty(max(p['ws_floats'] for p in plans), device=dev)
    maps = ra_fg_train._source_maps(sources[0], sources[0], sources[1] if len(sources) > 1 else 0, sources[1] if len(sources) > 1 else 0, dev)

    def wgrad():
      for k, x in enumerate(xs):
        ops.wgrad_wide_acc(x, du, gw, gb if k == 0 else None, chan_map=maps[1 + k], transposed=tr, upsample=bool(ups), ws=ws)

    tf, _, _ = timed(fwd)
    tg, lo, hi = timed(wgrad)
    # counted at the conv's own map: both kernels of a stride-2 layer walk the zero-stuffed image (three of four x positions are zeros)
    flop = 2.0 * 9 * cin * cout * B * Hs * Ws * up * up
    worst_ws = max(worst_ws, ws.numel() * 4)
    tot_f, tot_g = tot_f + tf, tot_g + tg
    emit('  %-4s %2d    %-13s  %4d  %3d x %-4d  %d  %7.2f   %9.1f  %5.1f   %8.1f [%.1f .. %.1f]  %5.1f  %5.1f %%      %5.2f   %-14s %6.1f' % (
        scope, i, '+'.join(map(str, sources)), cout, Hs, Ws, ups, flop / 1e9, tf, flop / tf / 1e6, tg, lo, hi, flop / tg / 1e6,
        100 * flop / (tg * 1e-6) / F32_MFMA_PEAK, tg / tf, ' + '.join('%d x %d' % (p['split'], p['tiles_per_part']) for p in plans), ws.numel() * 4 / 1e6))
  emit('  all wide layers: forward %.1f us, filter gradient %.1f us (ratio %.2f); largest filter-gradient workspace %.1f MB' % (
      tot_f, tot_g, tot_g / tot_f, worst_ws / 1e6))


def wide_main(args, emit):
  emit('python tools/fg_train_bench.py --wide%s — rounds %d, repetitions per round %d (median; steps: 9), warm-up %d (steps: 3); synthetic data' % (
      ' --small' if args.small else '', ROUNDS, REPS, WARM))
  wide_parity(emit)
  nets = (('run_kitti.sh', fo.kitti_opt(), (2, 64, 128) if args.small else (8, 128, 448)),
          ('run_cityscapes.sh', fo.cityscapes_opt(), (2, 64, 64) if args.small else (8, 256, 512)))
  for name, opt, shape in nets:
    wide_layers(emit, name, opt, *shape)
  emit('step: one FgTrainStep(model, wide=True).run, eager stream launches')
  for name, opt, shape in nets:
    step(emit, 'the net of ' + name, opt, *shape, wide=True)


def main():
  p = argparse.ArgumentParser()
  p.add_argument('--small', action='store_true', help='a rehearsal at toy sizes (numbers mean nothing)')
  p.add_argument('--wide', action='store_true', help='the wide path: the nets of run_kitti.sh and run_cityscapes.sh (profiles/fg_train_wide.txt)')
  p.add_argument('--out', default=None)
  args = p.parse_args()
  if args.out is None:
    args.out = os.path.join(HERE, '..', 'profiles', 'fg_train_wide.txt' if args.wide else 'fg_train.txt')
  if not torch.cuda.is_available():
    raise SystemExit('fg_train_bench needs an MI355X; there is nothing to time without one')
  lines = []

  def emit(line):
    print(line, flush=True)
    lines.append(line)

  if args.wide:
    wide_main(args, emit)
    with open(args.out, 'w') as f:
      f.write('\n'.join(lines) + '\n')
    return
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
