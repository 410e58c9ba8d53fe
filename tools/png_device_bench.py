#!/usr/bin/env python
"""PNG output with the deflate stage on the device against the host's zlib, one MI355X: png_device_bench.py [reps >= 5] [--out FILE].

Three images at 1024 x 2048, on the seeded one-label disc scene of tools/cityscapes_stage_bench.py:
  mask       one binary instance plane, float32 0 / 1 on the device (what RenderCityScapesOutputAnalyzer holds);
  masks x20  the T = 20 planes of one image in ONE call (the analyzer's call with --device_png);
  colour     one instance colour image, uint8 [1,H,W,3] from ops.render_instances.
Alternating in one process, per image
  (a) the device path end to end: utils/png.encode_gray8_dev / encode_colour8_dev — the launch chain of ra_png_deflate_u8, the
      copy of sizes and offsets, the copy of the used bytes, the host's wrap (CRC-32 of the stream) — wall clock around the call,
      the device idle before it;
  (b) the parent's path: the plane's quantisation and copy to the host ((y * 255).to(uint8).cpu().numpy(), img.cpu().numpy()) and
      utils/png.encode_gray8 / encode_colour8 at level 6, per plane as analysis.py does it — wall clock likewise;
`rounds` rounds, each a median of `reps` calls after a warm-up; printed: the median of the rounds and their spread (min .. max),
the bytes of the files, and (a) / (b).  (a) counts as faster when its whole spread lies below (b)'s.  Then the launch chain of (a)
alone between device events (no copy, no host work), and whether the files of (a) decode to the pixels of (b)'s."""
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'rec-attend-public_amd'))
import numpy as np

from cityscapes_stage_bench import scene


def main():
  import torch
  import ra_native as rn
  import ra_ops as ops
  from utils import png
  args = [a for a in sys.argv[1:] if not a.startswith('--')]
  reps = max(5, int(args[0])) if args else 7
  out_path = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else None
  if not torch.cuda.is_available():
    raise SystemExit('png_device_bench.py needs an MI355X')
  dev = torch.device('cuda:0')
  rounds, lines = 5, []

  def say(s):
    print(s, flush=True)
    lines.append(s)

  def wall_ms(fn):
    fn()
    ts = []
    for _ in range(reps):
      torch.cuda.synchronize()
      t0 = time.perf_counter()
      fn()
      ts.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ts))

  def events_us(fn):
    for _ in range(3):
      fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(21):
      e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      e0.record()
      fn()
      e1.record()
      e1.synchronize()
      ts.append(e0.elapsed_time(e1) * 1e3)
    return float(np.median(ts)), min(ts), max(ts)

  def chain(src, kind, bpp, planes=None):
    """The launch chain alone, on buffers allocated once: what ra_ops.png_deflate launches."""
    M, H, W = int(src.shape[0]), int(src.shape[1]), int(src.shape[2])
    N = M if planes is None else int(planes.numel())
    stream, ws_bytes = ops.png_deflate_bound(N, H, W, bpp)
    out = torch.empty((N * stream,), dtype=torch.uint8, device=dev)
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
    meta = torch.empty((4 * N,), dtype=torch.int32, device=dev)

    def run():
      rn.check(rn.lib().ra_png_deflate_u8(rn.ptr(src), kind, M, N, H, W, rn.ptr(planes), rn.ptr(out), out.numel(), rn.ptr(meta[:N]),
                                          rn.ptr(meta[2 * N:]), rn.ptr(meta[N:2 * N]), rn.ptr(ws), ws.numel(), rn.stream_ptr()),
               'ra_png_deflate_u8')
    return run, ws_bytes

  T, H, W = 20, 1024, 2048
  y = scene(np.random.RandomState(121), 1, T, H, W, dev)[0].contiguous()  # float32 [T,H,W] of 0 / 1
  areas = y.sum(dim=(1, 2))
  t_big = int(areas.argmax())
  colour = ops.render_instances(y[None])
  all_planes = torch.arange(T, dtype=torch.int32, device=dev)
  one_plane = torch.tensor([t_big], dtype=torch.int32, device=dev)

  def host_masks(ts):
    return [png.encode_gray8((y[t] * 255).to(torch.uint8).cpu().numpy()) for t in ts]

  cases = [
      ('mask', lambda: png.encode_gray8_dev(y, [t_big]), lambda: host_masks([t_big]), chain(y, rn.RA_PNG_F32, 1, one_plane), H * (W + 1)),
      ('masks x20', lambda: png.encode_gray8_dev(y, list(range(T))), lambda: host_masks(range(T)), chain(y, rn.RA_PNG_F32, 1, all_planes),
       T * H * (W + 1)),
      ('colour', lambda: png.encode_colour8_dev(colour), lambda: [png.encode_colour8(colour[0].cpu().numpy())],
       chain(colour, rn.RA_PNG_BGR8, 3), H * (3 * W + 1)),
  ]
  say('# %d x %d, T = %d one-label disc masks (largest plane: %.1f %% of the pixels); wall clock, %d rounds alternating, each a median of %d calls'
      % (H, W, T, 100.0 * float(areas.max()) / (H * W), rounds, reps))
  say('%-10s %-34s %10s %20s %12s %12s' % ('image', 'path', 'ms', 'spread (min..max)', 'file bytes', 'raw bytes'))
  for name, dev_fn, host_fn, (chain_fn, ws_bytes), raw in cases:
    fa, fb = dev_fn(), host_fn()
    same = len(fa) == len(fb) and all(np.array_equal(png.decode_colour8(a), png.decode_colour8(b)) for a, b in zip(fa, fb))
    ta, tb = [], []
    for _ in range(rounds):
      ta.append(wall_ms(dev_fn))
      tb.append(wall_ms(host_fn))
    ma, mb = float(np.median(ta)), float(np.median(tb))
    say('%-10s %-34s %10.3f %20s %12d %12d' % (name, '(a) device deflate, end to end', ma, '%.3f..%.3f' % (min(ta), max(ta)),
                                             sum(len(f) for f in fa), raw))
    say('%-10s %-34s %10.3f %20s %12d %12d' % (name, '(b) copy + host zlib level 6', mb, '%.3f..%.3f' % (min(tb), max(tb)),
                                             sum(len(f) for f in fb), raw))
    verdict = 'faster: its whole spread lies below (b)\'s' if max(ta) < min(tb) else (
        'slower: its whole spread lies above (b)\'s' if min(ta) > max(tb) else 'not separated: the spreads overlap')
    med, lo, hi = events_us(chain_fn)
    say('    %s: (a) / (b) = %.4f, (a) is %s; files (a) / (b) = %.2f; (a) decodes to (b)\'s pixels: %s' % (
        name, ma / mb, verdict, sum(len(f) for f in fa) / float(sum(len(f) for f in fb)), same))
    say('    %s: the launch chain alone (encode, scan, compact; device events, median of 21): %.1f us (%.1f..%.1f); workspace %.1f MB' % (
        name, med, lo, hi, ws_bytes * 1e-6))
  if out_path:
    with open(out_path, 'w') as f:
      f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
  main()
