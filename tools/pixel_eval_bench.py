#!/usr/bin/env python
"""Time of the Cityscapes pixel-level evaluation on one MI355X: pixel_eval_bench.py [reps >= 21] [--out FILE].

At B = 8, 1024 x 2048, on a generated instance-id image with about 60 instances per image (cityscapes_ap_bench.gt_scene), its
label image, and a nine-class semantic map at 256 x 512 (the pre-stage's 4x ratio; cs_oracle.smooth_semantic_map of a seed),
alternating in one process, the catalogue built once outside the timed calls:
  (a) label form   ops.pixel_confusion(labels uint8, ...)           ra_pixel_confusion_u8
  (b) arg-max      ops.sem_labels(sem, size)                          ra_sem_labels_u8
  (c) (b) then (a) the two launches one after the other
  (d) fused form   ops.pixel_confusion(sem, ..., size=)              ra_pixel_confusion_sem_f32
and the two confusion forms once more as the launches alone (the C entry points on buffers allocated once, without the ops
wrapper's workspace query and four allocations), `rounds` times, each a median of `reps` calls between device events after a warm-up.  (c) and (d) are compared for
equality.  Printed: the median of the rounds and their spread (min .. max), the bytes each form must read or write — gt_ids 4
+ gt_labels 1 + prediction 1 bytes per pixel for (a); the semantic map once + 1 byte per pixel written for (b); gt_ids 4 +
gt_labels 1 per pixel + the semantic map once for (d) — the time those bytes take at 8 TB/s (the floor), and the floor's share
of the measured time.  Then the same pass in NumPy on the host (np.add.at into a [34,34] matrix and the per-instance counts of
one image, times B), for scale."""
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '..', 'rec-attend-public_amd'))
sys.path.insert(0, os.path.join(HERE, '..', 'tests'))
sys.path.insert(0, os.path.join(HERE, '..', 'oracle'))
import numpy as np

from cityscapes_ap_bench import gt_scene

HBM_BYTES_PER_S = 8.0e12


def main():
  import torch
  import cs_oracle as cso
  import ra_ops as ops
  args = [a for a in sys.argv[1:] if not a.startswith('--')]
  reps = max(21, int(args[0])) if args else 21
  out_path = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else None
  if not torch.cuda.is_available():
    raise SystemExit('pixel_eval_bench.py needs an MI355X')
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

  B, H, W, Hs, Ws, C = 8, 1024, 2048, 256, 512, 9
  rng = np.random.RandomState(300)
  gt = gt_scene(rng, B, H, W, 60, dev)
  gl = torch.where(gt < 1000, gt, gt // 1000).to(torch.uint8).contiguous()
  sem = torch.from_numpy(cso.smooth_semantic_map(rng, B, Hs, Ws, C, bg_bias=2.0)).to(dev)
  cat = ops.gt_instance_catalog(gt)
  conf = torch.zeros((34, 34), dtype=torch.int64, device=dev)
  labels = ops.sem_labels(sem, (H, W))

  forms = [
      ('(a) label form', lambda: ops.pixel_confusion(labels, gt, gl, catalog=cat, conf=conf, check_status=False), B * H * W * 6.0),
      ('(b) sem_labels', lambda: ops.sem_labels(sem, (H, W)), B * (H * W * 1.0 + Hs * Ws * C * 4.0)),
      ('(c) sem_labels, then the label form',
       lambda: ops.pixel_confusion(ops.sem_labels(sem, (H, W)), gt, gl, catalog=cat, conf=conf, check_status=False),
       B * (H * W * 7.0 + Hs * Ws * C * 4.0)),
      ('(d) fused form', lambda: ops.pixel_confusion(sem, gt, gl, catalog=cat, size=(H, W), conf=conf, check_status=False),
       B * (H * W * 5.0 + Hs * Ws * C * 4.0)),
  ]
  # the launches alone, on buffers allocated once: what the ops wrapper (one workspace query, four allocations) adds is the difference
  import ra_native as rn
  from ra_native import ptr
  n_ws = rn.lib().ra_pixel_confusion_workspace_ints(B, H, W)
  ws = torch.empty((n_ws,), dtype=torch.int32, device=dev)
  itp, ictp = (torch.empty((B, ops.MAX_GT), dtype=torch.int32, device=dev) for _ in range(2))
  st = torch.empty((B,), dtype=torch.int32, device=dev)
  tail = (ptr(gt), ptr(gl), ptr(cat[0]), ptr(cat[2]), B, H, W, ptr(ws), n_ws, ptr(conf), ptr(itp), ptr(ictp), ptr(st))
  forms += [
      ('(a) launches alone', lambda: rn.lib().ra_pixel_confusion_u8(ptr(labels), *tail, rn.stream_ptr()), forms[0][2]),
      ('(d) launches alone', lambda: rn.lib().ra_pixel_confusion_sem_f32(ptr(sem), Hs, Ws, C, *tail, rn.stream_ptr()), forms[3][2]),
  ]
  c, d = forms[2][1](), forms[3][1]()
  same = all(bool(torch.equal(c[k], d[k])) for k in ('inst_tp', 'inst_cat_tp'))
  conf.zero_()
  forms[2][1]()
  conf_c = conf.clone()
  conf.zero_()
  forms[3][1]()
  same = same and bool(torch.equal(conf_c, conf)) and int(conf.sum()) == B * H * W
  times = [[] for _ in forms]
  for _ in range(rounds):
    for ts, (_, fn, _) in zip(times, forms):
      ts.append(median_us(fn))
  say('# pixel-level evaluation, B = %d, %d x %d, semantic map %d x %d x %d; about 60 instances per image (catalogue entries per '
      'image: %s); device events, %d rounds alternating the forms, each a median of %d calls (ops wrapper included: workspace '
      'and output allocation)' % (B, H, W, Hs, Ws, C, cat[2].tolist(), rounds, reps))
  say('%-40s %10s %20s %10s %10s %12s' % ('form', 'us', 'spread (min..max)', 'model MB', 'floor us', 'floor / time'))
  med = []
  for (name, _, nbytes), ts in zip(forms, times):
    m = float(np.median(ts))
    med.append(m)
    floor = nbytes / HBM_BYTES_PER_S * 1e6
    say('%-40s %10.1f %20s %10.1f %10.1f %11.1f%%' % (name, m, '%.1f..%.1f' % (min(ts), max(ts)), nbytes * 1e-6, floor, 100 * floor / m))
  say('(c) and (d) give equal counts: %s.  fused (d) / chain (c) = %.3f: the fused form is %s than sem_labels followed by the '
      'label form, by %.1f us' % (same, med[3] / med[2], 'faster' if med[3] < med[2] else 'NOT faster', abs(med[2] - med[3])))
  # the same pass in NumPy on the host, one image, times B
  lab_h, gt_h, gl_h = labels[0].cpu().numpy(), gt[0].cpu().numpy(), gl[0].cpu().numpy()
  t0 = time.perf_counter()
  m = np.zeros((34, 34), np.int64)
  np.add.at(m, (gl_h.ravel().astype(np.intp), lab_h.ravel().astype(np.intp)), 1)
  for inst in np.unique(gt_h[gt_h > 1000]):
    mask = gt_h == inst
    (lab_h[mask] == inst // 1000).sum()
  host = time.perf_counter() - t0
  say('NumPy on the host (np.add.at into [34,34] + one mask per instance), one image: %.0f ms; times B = %d: %.0f ms = %.0f x the '
      'label form' % (host * 1e3, B, host * B * 1e3, host * B * 1e6 / med[0]))
  if out_path:
    with open(out_path, 'w') as f:
      f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
  main()
