#!/usr/bin/env python
"""PNG output with the deflate stage on the device against the host's zlib, one MI355X: png_device_bench.py [reps >= 5] [--out FILE].

Three images at 1024 x 2048, on the seeded one-label disc scene of tools/cityscapes_stage_bench.py:
  mask       one binary instance plane, float32 0 / 1 on the device (what RenderCityScapesOutputAnalyzer holds);
  masks x20  the T = 20 planes of one image in ONE call (the analyzer's call with --device_png);
  colour     one instance colour image, uint8 [1,H,W,3] from ops.render_instances.
Alternating in one process, per image, with the stream format in the `code` column
  (a) dynamic  the device path end to end with code='dynamic' (ra_png_deflate_dyn_u8: one dynamic-Huffman block per image):
               utils/png.encode_gray8_dev / encode_colour8_dev — the launch chain, the copy of sizes and offsets, the copy of the
               used bytes, the host's wrap (CRC-32 of the stream) — wall clock around the call, the device idle before it;
  (b) fixed    the same with code='fixed' (ra_png_deflate_u8: a fixed-Huffman block per row), the default;
  (c) zlib     the host's path: the plane's quantisation and copy to the host ((y * 255).to(uint8).cpu().numpy(),
               img.cpu().numpy()) and utils/png.encode_gray8 / encode_colour8 at level 6, per plane as analysis.py does it.
`rounds` rounds, each a median of `reps` calls after a warm-up; printed: the median of the rounds and their spread (min .. max),
the bytes of the files, and the ratios.  A path counts as faster than another when its whole spread lies below the other's.  Then
the launch chains of (a) and (b) alone between device events (no copy, no host work) with their workspaces, and whether the
files of (a) and (b) decode to the pixels of (c)'s."""
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

  def chain(src, kind, bpp, code, planes=None):
    """The launch chain of the stream format `code` alone, on buffers allocated once: what ra_ops.png_deflate launches."""
    M, H, W = int(src.shape[0]), int(src.shape[1]), int(src.shape[2])
    N = M if planes is None else int(planes.numel())
    stream, ws_bytes = ops.png_deflate_bound(N, H, W, bpp, code)
    out = torch.empty((N * stream,), dtype=torch.uint8, device=dev)
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
    meta = torch.empty((4 * N,), dtype=torch.int32, device=dev)
    name = ops.PNG_CODES[code] + '_u8'
    entry = getattr(rn.lib(), name)

    def run():
      rn.check(entry(rn.ptr(src), kind, M, N, H, W, rn.ptr(planes), rn.ptr(out), out.numel(), rn.ptr(meta[:N]), rn.ptr(meta[2 * N:]),
                     rn.ptr(meta[N:2 * N]), rn.ptr(ws), ws.numel(), rn.stream_ptr()), name)
    return run, ws_bytes, N * stream

  T, H, W = 20, 1024, 2048
  y = scene(np.random.RandomState(121), 1, T, H, W, dev)[0].contiguous()  # float32 [T,H,W] of 0 / 1
  areas = y.sum(dim=(1, 2))
  t_big = int(areas.argmax())
  colour = ops.render_instances(y[None])
  all_planes = torch.arange(T, dtype=torch.int32, device=dev)
  one_plane = torch.tensor([t_big], dtype=torch.int32, device=dev)

  def host_masks(ts):
    return [png.encode_gray8((y[t] * 255).to(torch.uint8).cpu().numpy()) for t in ts]

  codes = ('dynamic', 'fixed')
  cases = [
      ('mask', lambda c: png.encode_gray8_dev(y, [t_big], code=c), lambda: host_masks([t_big]),
       lambda c: chain(y, rn.RA_PNG_F32, 1, c, one_plane), H * (W + 1)),
      ('masks x20', lambda c: png.encode_gray8_dev(y, list(range(T)), code=c), lambda: host_masks(range(T)),
       lambda c: chain(y, rn.RA_PNG_F32, 1, c, all_planes), T * H * (W + 1)),
      ('colour', lambda c: png.encode_colour8_dev(colour, code=c), lambda: [png.encode_colour8(colour[0].cpu().numpy())],
       lambda c: chain(colour, rn.RA_PNG_BGR8, 3, c), H * (3 * W + 1)),
  ]
  say('# %d x %d, T = %d one-label disc masks (largest plane: %.1f %% of the pixels); wall clock, %d rounds alternating, each a median of %d calls'
      % (H, W, T, 100.0 * float(areas.max()) / (H * W), rounds, reps))
  say('%-10s %-8s %-34s %10s %20s %12s %12s' % ('image', 'code', 'path', 'ms', 'spread (min..max)', 'file bytes', 'raw bytes'))

  def verdict(ta, tb):
    return 'faster: its whole spread lies below' if max(ta) < min(tb) else (
        'slower: its whole spread lies above' if min(ta) > max(tb) else 'not separated: the spreads overlap')

  for name, dev_fn, host_fn, chain_of, raw in cases:
    files = {c: dev_fn(c) for c in codes}
    files['zlib'] = host_fn()
    same = {c: len(files[c]) == len(files['zlib']) and all(np.array_equal(png.decode_colour8(a), png.decode_colour8(b))
                                                            for a, b in zip(files[c], files['zlib'])) for c in codes}
    ts = {c: [] for c in codes + ('zlib',)}
    for _ in range(rounds):
      for c in codes:
        ts[c].append(wall_ms(lambda: dev_fn(c)))
      ts['zlib'].append(wall_ms(host_fn))
    med = {c: float(np.median(v)) for c, v in ts.items()}
    size = {c: sum(len(f) for f in v) for c, v in files.items()}
    for tag, c, what in (('(a)', 'dynamic', 'device deflate, end to end'), ('(b)', 'fixed', 'device deflate, end to end'),
                         ('(c)', 'zlib', 'copy + host zlib level 6')):
      say('%-10s %-8s %-34s %10.3f %20s %12d %12d' % (name, c, tag + ' ' + what, med[c], '%.3f..%.3f' % (min(ts[c]), max(ts[c])), size[c], raw))
    say('    %s: (a) / (c) = %.4f, (a) is %s (c)\'s; (a) / (b) = %.3f, (a) is %s (b)\'s' % (
        name, med['dynamic'] / med['zlib'], verdict(ts['dynamic'], ts['zlib']), med['dynamic'] / med['fixed'],
        verdict(ts['dynamic'], ts['fixed'])))
    say('    %s: files (a) / (b) = %.3f, (a) / (c) = %.3f, (b) / (c) = %.2f; decode to (c)\'s pixels: (a) %s, (b) %s' % (
        name, size['dynamic'] / float(size['fixed']), size['dynamic'] / float(size['zlib']), size['fixed'] / float(size['zlib']),
        same['dynamic'], same['fixed']))
    for c in codes:
      chain_fn, ws_bytes, out_bytes = chain_of(c)
      m, lo, hi = events_us(chain_fn)
      say('    %s: the %s launch chain alone (device events, median of 21): %.1f us (%.1f..%.1f); workspace %.1f MB, output buffer %.1f MB' % (
          name, c, m, lo, hi, ws_bytes * 1e-6, out_bytes * 1e-6))
      del chain_fn
      torch.cuda.empty_cache()
  if out_path:
    with open(out_path, 'w') as f:
      f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
  main()
