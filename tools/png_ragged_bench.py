#!/usr/bin/env python
"""A batch of MIXED sizes through the device PNG encoder, one MI355X: png_ragged_bench.py [rounds >= 21] [--out FILE].

B = 8 images of four KITTI sizes in mixed order, as seeded disc scenes of T = 20 instances:
  colour K=1    one flat-colour picture per image, uint8 [1,P,3] as ops.paint_instances(..., geo=...) lays it out;
  colour K=10   ten pictures per image (ten thresholds: the discs shrink), [10,P,3];
  masks  K=10   ten binary planes per image, uint8 [10,P] of 0 / 255 (fg_model_eval.py's thresholded planes).
Per case and stream format, alternating in one process, wall clock around the whole call with the device idle before it (the
launch chains, the copies of metadata and bytes, the host's wrap):
  (a) ragged    ONE utils/png.encode_*_ragged_dev call on the flat buffer;
  (a1) ragged, a call per plane   K calls of one plane each: what the render analyzers do, which stage one threshold at a time;
  (b) grouped   the route before the ragged entry: per plane the views of equal size are torch.stack-ed into a fresh tensor and
                every group is one uniform utils/png.encode_*_dev call.
Then a batch of ONE size (8 x 375 x 1242), ragged against ONE uniform call on the same memory: the fixed cost of the table.
Printed: the median of the rounds and their spread (min .. max); a route counts as faster when its whole spread lies below the
other's.  The files of (a) and (b) are compared byte for byte.  Last, the encode stage's load width: the ragged launch chain alone
(device events, no copies) on 8 x 375 x 1242 (KITTI: 1242 % 16 != 0, element loads) against 8 x 375 x 1248 (16-byte loads)."""
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'rec-attend-public_amd'))
import numpy as np

KITTI = ((375, 1242), (370, 1224), (374, 1238), (376, 1241))
ORDER = (0, 1, 2, 0, 3, 1, 0, 2)
T = 20


def scene(rng, h, w, K):
  """uint8 [K,h,w] of labels 0 .. T: T discs, plane k with the radii shrunk by 3 k %."""
  rr, cc = np.mgrid[0:h, 0:w]
  cy, cx, rad = rng.uniform(20, h - 20, T), rng.uniform(20, w - 20, T), rng.uniform(15, 70, T)
  out = np.zeros((K, h, w), np.uint8)
  for k in range(K):
    for t in range(T):
      out[k][(rr - cy[t]) ** 2 + (cc - cx[t]) ** 2 <= (rad[t] * (1.0 - 0.03 * k)) ** 2] = t + 1
  return out


def main():
  import torch
  import ra_native as rn
  import ra_ops as ops
  from utils import png
  argv = sys.argv[1:]
  out_path = None
  if '--out' in argv:
    at = argv.index('--out')
    out_path = argv[at + 1]
    del argv[at:at + 2]
  rounds = max(21, int(argv[0])) if argv else 21
  if not torch.cuda.is_available():
    raise SystemExit('png_ragged_bench.py needs an MI355X')
  dev = torch.device('cuda:0')
  lines = []

  def say(s):
    print(s, flush=True)
    lines.append(s)

  rng = np.random.RandomState(131)
  palette = np.concatenate([np.zeros((1, 3), np.uint8), rng.randint(1, 256, size=(T, 3)).astype(np.uint8)])

  def batch(sizes, K, align=ops.RAGGED_ALIGN):
    """(labels uint8 [K,P] on the device, geometry) of the seeded scenes of the given sizes."""
    geo, total = ops.ragged_geometry(sizes, align)
    flat = np.zeros((K, total), np.uint8)
    for (o, h, w) in geo.tolist():
      flat[:, o:o + h * w] = scene(rng, h, w, K).reshape(K, -1)
    return torch.from_numpy(flat).to(dev), geo

  def grouped(flat, geo, colour, code):
    """The route before the ragged entry: per plane, one stacked uniform call per group of equal size; files in stream order."""
    files = []
    for plane in flat:
      views = [plane[o:o + h * w].view((h, w, 3) if colour else (h, w)) for o, h, w in geo.tolist()]
      groups = {}
      for ii, v in enumerate(views):
        groups.setdefault(tuple(v.shape), []).append(ii)
      got = [None] * len(views)
      for members in groups.values():
        stack = torch.stack([views[ii] for ii in members])
        for ii, f in zip(members, png.encode_colour8_dev(stack, code=code) if colour else png.encode_gray8_dev(stack, code=code)):
          got[ii] = f
      files += got
    return files

  def alternate(fns):
    """{name: [ms per round]}: every round runs each route once, sync-bracketed, after two warm-up rounds."""
    ts = {n: [] for n in fns}
    for r in range(rounds + 2):
      for n, fn in fns.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        if r >= 2:
          ts[n].append(1e3 * (time.perf_counter() - t0))
    return ts

  def verdict(ta, tb):
    return 'faster: its whole spread lies below' if max(ta) < min(tb) else (
        'slower: its whole spread lies above' if min(ta) > max(tb) else 'not separated: the spreads overlap')

  def report(case, code, ts, notes):
    for n, v in ts.items():
      say('%-13s %-8s %-32s %9.3f %18s' % (case, code, n, float(np.median(v)), '%.3f..%.3f' % (min(v), max(v))))
    for s in notes:
      say('    ' + s)

  say('# B = 8 of four KITTI sizes %s in the order %s, T = %d flat-colour discs; wall clock end to end, %d rounds alternating after 2 of warm-up'
      % (KITTI, ORDER, T, rounds))
  say('%-13s %-8s %-32s %9s %18s' % ('case', 'code', 'route', 'median ms', 'spread (min..max)'))
  mixed = [KITTI[i] for i in ORDER]
  for case, K, colour in (('colour K=1', 1, True), ('colour K=10', 10, True), ('masks K=10', 10, False)):
    labels, geo = batch(mixed, K)
    flat = torch.from_numpy(palette).to(dev)[labels.long()].contiguous() if colour else ((labels > 0).to(torch.uint8) * 255).contiguous()
    enc = png.encode_colour8_ragged_dev if colour else png.encode_gray8_ragged_dev
    for code in ('fixed', 'dynamic'):
      a, b = enc(flat, geo, code=code), grouped(flat, geo, colour, code)
      fns = {'(a) ragged, one call': lambda: enc(flat, geo, code=code)}
      if K > 1:
        fns['(a1) ragged, a call per plane'] = lambda: [enc(p, geo, code=code) for p in flat]
      fns['(b) grouped uniform calls'] = lambda: grouped(flat, geo, colour, code)
      ts = alternate(fns)
      ta, tb = ts['(a) ragged, one call'], ts['(b) grouped uniform calls']
      notes = ['%s %s: (a) / (b) = %.3f, (a) is %s (b)\'s; %d files, %d bytes, (a) == (b) byte for byte: %s' % (
          case, code, np.median(ta) / np.median(tb), verdict(ta, tb), len(a), sum(len(f) for f in a), a == b)]
      if K > 1:
        t1 = ts['(a1) ragged, a call per plane']
        notes.append('%s %s: (a1) / (b) = %.3f, (a1) is %s (b)\'s' % (case, code, np.median(t1) / np.median(tb), verdict(t1, tb)))
      report(case, code, ts, notes)
    del labels, flat
    torch.cuda.empty_cache()

  say('# one size: B = 8 of %d x %d, colour K=1 — ragged against ONE uniform call on the same memory (no stack): the table\'s fixed cost' % KITTI[0])
  labels, geo = batch([KITTI[0]] * 8, 1, align=1)
  flat = torch.from_numpy(palette).to(dev)[labels.long()].contiguous()
  assert geo[1, 0] == KITTI[0][0] * KITTI[0][1]  # no padding between the images: the flat buffer IS [8,H,W,3]
  uni = flat.view(8, KITTI[0][0], KITTI[0][1], 3)
  for code in ('fixed', 'dynamic'):
    same = png.encode_colour8_ragged_dev(flat, geo, code=code) == png.encode_colour8_dev(uni, code=code)
    ts = alternate({'(a) ragged, one call': lambda: png.encode_colour8_ragged_dev(flat, geo, code=code),
                    '(u) uniform, one call': lambda: png.encode_colour8_dev(uni, code=code)})
    ta, tu = ts['(a) ragged, one call'], ts['(u) uniform, one call']
    report('one size', code, ts, ['one size %s: (a) / (u) = %.3f, (a) is %s (u)\'s; byte for byte: %s' % (
        code, np.median(ta) / np.median(tu), verdict(ta, tu), same)])

  say('# the load width of the encode stage: the ragged launch chain alone (device events, median of 21, no copies), colour, B = 8')

  def chain_us(w, code):
    lab, g = batch([(375, w)] * 8, 1)
    src = torch.from_numpy(palette).to(dev)[lab.long()].contiguous()
    tab, gdev, B, total = ops._geo_table('png_ragged_bench', g, (src.view(-1)[:src.shape[1]],), dev)
    out_bytes, ws_bytes = ops.png_deflate_ragged_bound(g, 1, 3, code)
    out = torch.empty((out_bytes,), dtype=torch.uint8, device=dev)
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
    meta = torch.empty((4 * B,), dtype=torch.int32, device=dev)
    name = ops.PNG_CODES[code] + '_ragged_u8'
    entry = getattr(rn.lib(), name)

    def run():
      rn.check(entry(rn.ptr(src), rn.RA_PNG_BGR8, 1, total, tab, rn.ptr(gdev), B, None, 1, rn.ptr(out), out.numel(), rn.ptr(meta[:B]),
                     rn.ptr(meta[2 * B:]), rn.ptr(meta[B:2 * B]), rn.ptr(ws), ws.numel(), rn.stream_ptr()), name)
    for _ in range(3):
      run()
    torch.cuda.synchronize()
    ts = []
    for _ in range(21):
      e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      e0.record()
      run()
      e1.record()
      e1.synchronize()
      ts.append(e0.elapsed_time(e1) * 1e3)
    return float(np.median(ts)), min(ts), max(ts), ws_bytes

  for code in ('fixed', 'dynamic'):
    for w, what in ((1242, 'element loads (1242 % 16 = 10)'), (1248, '16-byte loads')):
      m, lo, hi, ws_bytes = chain_us(w, code)
      say('%-8s 8 x 375 x %d  %-32s %8.1f us (%.1f..%.1f)  %.2f ns per pixel  workspace %.1f MB' % (
          code, w, what, m, lo, hi, 1e3 * m / (8 * 375 * w), ws_bytes * 1e-6))
  ws_mixed = ops.png_deflate_ragged_bound(ops.ragged_geometry(mixed)[0], 1, 3, 'fixed')[1]
  ws_own = sum(ops.png_deflate_bound(1, h, w, 3, 'fixed')[1] for h, w in mixed)
  say('# workspace of the mixed batch (fixed, colour, K=1): %d bytes, sized by the tallest and widest image; the images\' own: %d (+%.2f %%)'
      % (ws_mixed, ws_own, 100.0 * (ws_mixed - ws_own) / ws_own))
  if out_path:
    with open(out_path, 'w') as f:
      f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
  main()
