#!/usr/bin/env python
"""Time of the label stage on one MI355X: labels_bench.py [reps >= 21] [--out FILE] [--no-train] [--no-host].

At the Cityscapes operating point — B = 8 id images of 1024 x 2048 sampled to 256 x 512, T = 20, the Cityscapes rule, every
output — on a seeded scene (ellipses whose ids are labelId * 1000 + k over stuff bands), `rounds` times, each a median of
`reps` calls between device events after a warm-up:
  (a) ra_ops.assemble_labels: the catalogue of the full-size image, the stage's launches, the status check (one
      device-to-host copy) and the wrapper's allocations;
  (b) ra_ops.assemble_labels_raw on a catalogue made once: the stage's launches alone;
  (c) ra_ops.gt_instance_catalog alone.
Printed with each: the bytes the stage must move at least — the sampled ids in, y_gt, d_gt, c_gt and fg_gt_full out, the
full-size ids once for fg_gt_full and (for (a) and (c)) once for the catalogue — and the share of the 8 TB/s HBM peak those
bytes make of the measured time.  Then the wall time of tests/labels_oracle.py on the same batch on the host, the stand-in
for the reference's stage, after the device outputs have been compared with it.

Unless --no-train: one training step at cfg4 shapes (bench.py --train: CVPPP architecture, 512 x 512, T = 16, B = 8) fed
pre-assembled planes against the same step fed ids, the eager assembly in front of the captured step timed on its own."""
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
for p in (os.path.join(ROOT, 'rec-attend-public_amd'), os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'oracle'), ROOT):
  sys.path.insert(0, p)
import numpy as np

HBM_BYTES_PER_S = 8.0e12


def scene(rng, B, Hf, Wf, n_inst):
  """int32 [B,Hf,Wf]: road and sky bands (stuff ids 7, 23), n_inst ellipses of the eight instance labels, every tenth a
  caravan (29); painted row by row so that no full-size float plane is needed."""
  labels = (24, 25, 26, 27, 28, 31, 32, 33)
  gt = np.zeros((B, Hf, Wf), np.int32)
  cc = np.arange(Wf, dtype=np.float64)[None, :]
  for b in range(B):
    gt[b, : Hf // 4] = 23
    gt[b, Hf - Hf // 3:] = 7
    for k in range(n_inst):
      ry, rx = rng.uniform(0.02, 0.12) * Hf, rng.uniform(0.02, 0.12) * Wf
      cy, cx = rng.uniform(0.2, 0.9) * Hf, rng.uniform(0, 1) * Wf
      r0, r1 = max(0, int(cy - ry)), min(Hf, int(cy + ry) + 1)
      rr = np.arange(r0, r1, dtype=np.float64)[:, None]
      label = 29 if k % 10 == 9 else labels[rng.randint(len(labels))]
      gt[b, r0:r1][((rr - cy) / ry) ** 2 + ((cc - cx) / rx) ** 2 <= 1.0] = label * 1000 + k
  return gt


def main():
  import torch
  import ra_ops as ops
  args = [a for a in sys.argv[1:] if not a.startswith('--')]
  reps = max(21, int(args[0])) if args else 31
  out_path = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else None
  if not torch.cuda.is_available():
    raise SystemExit('labels_bench.py needs an MI355X')
  dev = torch.device('cuda:0')
  rounds, lines = 5, []

  def say(s):
    print(s, flush=True)
    lines.append(s)

  def median_us(fn, n=reps):
    for _ in range(5):
      fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(n):
      e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      e0.record()
      fn()
      e1.record()
      e1.synchronize()
      ts.append(e0.elapsed_time(e1) * 1e3)
    return float(np.median(ts))

  B, Hf, Wf, H, W, T, nc = 8, 1024, 2048, 256, 512, 20, 9
  gt_host = scene(np.random.RandomState(1), B, Hf, Wf, 40)
  gt = torch.from_numpy(gt_host).to(dev)
  cat = ops.gt_instance_catalog(gt)
  full = lambda: ops.assemble_labels(gt, H, W, T, 'cityscapes', want=ops.LABEL_OUTPUTS)
  raw = lambda: ops.assemble_labels_raw(gt, cat, H, W, T, 'cityscapes', want=ops.LABEL_OUTPUTS)
  catalogue = lambda: ops.gt_instance_catalog(gt)
  out_bytes = 4.0 * B * H * W * (T + 8 + nc) + 1.0 * B * Hf * Wf
  stage_bytes = 4.0 * B * H * W + out_bytes + 4.0 * B * Hf * Wf  # sampled ids, the outputs, the full-size ids for fg_gt_full
  cat_bytes = 4.0 * B * Hf * Wf
  say('# label stage, B = %d, %d x %d -> %d x %d, T = %d, Cityscapes rule, all outputs; %d instances per image in the catalogue '
      '(max); device events, %d rounds, each a median of %d' % (B, Hf, Wf, H, W, T, int(cat[2].max()), rounds, reps))
  say('%-58s %10s %18s %10s %12s' % ('form', 'us', 'spread (min..max)', 'least MB', '% of 8 TB/s'))
  ts = {'a': [], 'b': [], 'c': []}
  for _ in range(rounds):
    ts['a'].append(median_us(full))
    ts['b'].append(median_us(raw))
    ts['c'].append(median_us(catalogue))
  for key, name, nbytes in (('a', '(a) assemble_labels: catalogue + stage + status check', stage_bytes + cat_bytes),
                            ('b', '(b) assemble_labels_raw: the stage alone', stage_bytes), ('c', '(c) gt_instance_catalog alone', cat_bytes)):
    med = float(np.median(ts[key]))
    say('%-58s %10.1f %18s %10.1f %12.1f' % (name, med, '%.1f..%.1f' % (min(ts[key]), max(ts[key])), nbytes * 1e-6,
                                             100 * nbytes / (med * 1e-6) / HBM_BYTES_PER_S))
  got = {k: v.cpu().numpy() for k, v in full().items()}
  del gt
  if '--no-host' not in sys.argv:
    import labels_oracle as lo
    t0 = time.perf_counter()
    ref = lo.assemble(gt_host, H, W, T, lo.CITYSCAPES)
    host_s = time.perf_counter() - t0
    same = all(np.array_equal(got[k], ref[k]) for k in lo.KEYS)
    say('    host: tests/labels_oracle.py (NumPy float64, one thread of control) on the same batch: %.2f s wall = %.0f x (a); its '
        'outputs %s the device\'s (orientation margin of the oracle %.3g)' % (
            host_s, host_s / (float(np.median(ts['a'])) * 1e-6), 'EQUAL' if same else 'DIFFER FROM', ref['ori_margin']))
  if '--no-train' not in sys.argv:
    train_lines(say, median_us, dev)
  if out_path:
    with open(out_path, 'w') as f:
      f.write('\n'.join(lines) + '\n')


def train_lines(say, median_us, dev):
  """One cfg4 training step from planes against the same step from ids."""
  import torch
  import bench
  import full_model
  import full_model_train as fmt
  import ra_ops as ops
  B, S, T = 8, 512, 16
  opt = bench.make_opt('cvppp', S, S, T)
  opt.update(use_knob=True, knob_base=1.0, knob_decay=0.9, steps_per_knob_decay=300, knob_box_offset=300, knob_segm_offset=500,
             knob_use_timescale=True, gt_box_ctr_noise=0.05, gt_box_pad_noise=0.1, gt_segm_noise=0.3, base_learn_rate=1e-3,
             learn_rate_decay=0.96, steps_per_learn_rate_decay=5000, sync_bn=False, seed=1234, compute_dtype='float32')
  model = full_model.get_model(opt, is_training=True)
  x, y, _ = fmt.synthetic_batch(np.random.RandomState(1234), B, S, S, T)
  ids = np.zeros((B, S, S), np.int32)
  for t in range(T - 1, -1, -1):  # the largest painted last: every instance keeps pixels
    ids[y[:, t] > 0] = t + 1
  gt = torch.from_numpy(ids).to(dev)
  planes = ops.assemble_labels(gt, S, S, T, 'cvppp')
  gen = torch.Generator(device='cuda').manual_seed(1234)
  feed = {'x': torch.as_tensor(x).to(dev), 'y_gt': planes['y_gt'], 's_gt': planes['s_gt'], 'phase_train': True, 'generator': gen}

  def step_planes():
    model.run(['loss', 'train_step'], feed)

  def assemble():
    return ops.assemble_labels(gt, S, S, T, 'cvppp')

  def step_ids():
    got = assemble()
    model.run(['loss', 'train_step'], dict(feed, y_gt=got['y_gt'], s_gt=got['s_gt']))

  for _ in range(3):  # the first step of a shape runs eagerly, the second is captured
    step_planes()
  rows = [('training step from pre-assembled planes', step_planes), ('the eager assembly in front of it (ids 512 x 512 -> y_gt, s_gt)', assemble),
          ('training step from ids (assembly + step)', step_ids)]
  say('# one training step at cfg4 shapes (CVPPP architecture, %d x %d, T = %d, B = %d, float32); device events, 3 rounds, each a median '
      'of 11' % (S, S, T, B))
  for name, fn in rows:
    t = [median_us(fn, 11) for _ in range(3)]
    say('%-66s %10.2f ms   (%.2f..%.2f)' % (name, float(np.median(t)) * 1e-3, min(t) * 1e-3, max(t) * 1e-3))
  model.trainer.flush_status()


if __name__ == '__main__':
  main()
