#!/usr/bin/env python
"""Time of the image stage on one MI355X: image_stage_bench.py [reps >= 21] [--out FILE] [--no-host] [--no-png].

At the Cityscapes point — B = 8 colour images of 1024 x 2048 x 3 resized to 256 x 512, float32 x out — and at KITTI's — B = 8
of 375 x 1242 x 3 to 128 x 448 — on seeded uniform-random uint8, `rounds` times, each a median of `reps` calls between device
events after a warm-up:
  (a) ra_resize_cubic_u8 alone, through the C ABI on tensors and tables made once;
  (b) ra_ops.resize_cubic on a device tensor: the same launch with the wrapper's allocation of x.
Printed with each: the bytes the kernel must move at least — every source byte the taps touch once, x once — and the share
of the 8 TB/s HBM peak those bytes make of the measured time (the bound of this kernel is bandwidth).  Then the wall time of
tests/image_oracle.py (NumPy) on the same batch on the host, after the device's output has been compared with it.

Unless --no-png: utils/png.decode_colour8 on one 1024 x 2048 RGB file whose rows all use the Paeth filter, through the
compiled unfilter (ra_png_unfilter_u8) and through the NumPy anti-diagonals, host wall time, best of 3."""
import os
import sys
import time
import zlib

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
for p in (os.path.join(ROOT, 'rec-attend-public_amd'), os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'oracle'), ROOT):
  sys.path.insert(0, p)
import numpy as np

HBM_BYTES_PER_S = 8.0e12
POINTS = (('Cityscapes', 8, 1024, 2048, 256, 512), ('KITTI', 8, 375, 1242, 128, 448))


def touched(S, D):
  """Source indices of one axis that some tap reads."""
  import image_oracle as io_
  ofs, _ = io_.cubic_table(S, D)
  return len(np.unique(np.clip(ofs[:, None] - 1 + np.arange(4)[None, :], 0, S - 1)))


def paeth_png(img):
  """An RGB PNG of img uint8 [H,W,3] with filter type 4 on every row, filtered with NumPy a row at a time."""
  from utils import png
  H, W, _ = img.shape
  cur = img.reshape(H, W * 3).astype(np.int64)
  up = np.vstack([np.zeros((1, W * 3), np.int64), cur[:-1]])
  a = np.hstack([np.zeros((H, 3), np.int64), cur[:, :-3]])
  c = np.hstack([np.zeros((H, 3), np.int64), up[:, :-3]])
  pa, pb, pc = np.abs(up - c), np.abs(a - c), np.abs(a + up - 2 * c)
  pred = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, up, c))
  rows = np.full((H, W * 3 + 1), 4, np.uint8)
  rows[:, 1:] = ((cur - pred) & 255).astype(np.uint8)
  import struct
  return (png.SIGNATURE + png._chunk(b'IHDR', struct.pack('>IIBBBBB', W, H, 8, 2, 0, 0, 0)) +
          png._chunk(b'IDAT', zlib.compress(rows.tobytes(), 1)) + png._chunk(b'IEND', b''))


def png_lines(say):
  from utils import png
  rng = np.random.RandomState(3)
  # a smooth image with noise, so that the file is no constant and Paeth predicts something
  yy, xx = np.mgrid[0:1024, 0:2048]
  img = np.stack([(yy // 4 + xx // 8) % 256, (yy // 2) % 256, (xx // 3) % 256], axis=2).astype(np.uint8) ^ rng.randint(0, 8, size=(1024, 2048, 3)).astype(np.uint8)
  data = paeth_png(img)
  if not png._native():
    raise SystemExit('image_stage_bench.py: librecattend.so cannot be loaded; build it first')

  def best(n):
    ts = []
    for _ in range(n):
      t0 = time.perf_counter()
      got = png.decode_colour8(data)
      ts.append(time.perf_counter() - t0)
    return min(ts), got

  t_native, got = best(3)
  same = np.array_equal(got, img[:, :, ::-1])
  saved = png._NATIVE[:]
  png._NATIVE[:] = [None]
  try:
    t_numpy, got2 = best(1)
  finally:
    png._NATIVE[:] = saved
  say('# utils/png.decode_colour8, one 1024 x 2048 RGB file, Paeth filter on every row (%.1f MB of file), host wall time' % (len(data) * 1e-6))
  say('  compiled unfilter (ra_png_unfilter_u8): %.1f ms (best of 3), inflate included; pixels %s the image that was encoded' % (
      t_native * 1e3, 'EQUAL' if same else 'DIFFER FROM'))
  say('  NumPy anti-diagonals (_unfilter_diagonals): %.1f ms (one run) = %.0f x; pixels %s' % (
      t_numpy * 1e3, t_numpy / t_native, 'EQUAL' if np.array_equal(got, got2) else 'DIFFER'))


def main():
  import torch
  import image_oracle as io_
  import ra_native as rn
  import ra_ops as ops
  out_path = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else None
  args = [a for a in sys.argv[1:] if not a.startswith('--') and a != out_path]
  reps = max(21, int(args[0])) if args else 31
  if not torch.cuda.is_available():
    raise SystemExit('image_stage_bench.py needs an MI355X')
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

  say('# image stage: ra_resize_cubic_u8, uint8 [B,Hs,Ws,3] -> x float32 [B,H,W,3]; device events, %d rounds, each a median of %d' % (rounds, reps))
  say('%-12s %-44s %10s %18s %10s %12s' % ('point', 'form', 'us', 'spread (min..max)', 'least MB', '% of 8 TB/s'))
  for name, B, Hs, Ws, H, W in POINTS:
    host = np.random.RandomState(1).randint(0, 256, size=(B, Hs, Ws, 3)).astype(np.uint8)
    src = torch.from_numpy(host).to(dev)
    oy, cy = ops._cubic_tables_dev(Hs, H, dev)
    ox, cx = ops._cubic_tables_dev(Ws, W, dev)
    x = torch.empty((B, H, W, 3), dtype=torch.float32, device=dev)
    lib, st = rn.lib(), rn.stream_ptr()

    def kernel():
      rn.check(lib.ra_resize_cubic_u8(src.data_ptr(), B, Hs, Ws, 3, H, W, oy.data_ptr(), cy.data_ptr(), ox.data_ptr(), cx.data_ptr(),
                                      None, x.data_ptr(), st), 'ra_resize_cubic_u8')

    wrapper = lambda: ops.resize_cubic(src, H, W)
    in_bytes = 3.0 * B * touched(Hs, H) * touched(Ws, W)
    nbytes = in_bytes + 4.0 * B * H * W * 3
    ts = {'a': [], 'b': []}
    for _ in range(rounds):
      ts['a'].append(median_us(kernel))
      ts['b'].append(median_us(wrapper))
    for key, form in (('a', '(a) ra_resize_cubic_u8 alone'), ('b', '(b) ra_ops.resize_cubic with its allocation')):
      med = float(np.median(ts[key]))
      say('%-12s %-44s %10.1f %18s %10.1f %12.1f' % (name, form, med, '%.1f..%.1f' % (min(ts[key]), max(ts[key])), nbytes * 1e-6,
                                                     100 * nbytes / (med * 1e-6) / HBM_BYTES_PER_S))
    say('%-12s   B = %d, %d x %d -> %d x %d: %.1f MB in (the source bytes some tap reads, of %.1f MB), %.1f MB out' % (
        '', B, Hs, Ws, H, W, in_bytes * 1e-6, 3.0 * B * Hs * Ws * 1e-6, 4.0 * B * H * W * 3 * 1e-6))
    got = ops.resize_cubic(src, H, W, want=('x', 'u8'))
    if '--no-host' not in sys.argv:
      t0 = time.perf_counter()
      ref = io_.resize_cubic_u8(host, H, W)
      host_s = time.perf_counter() - t0
      same = np.array_equal(got['u8'].cpu().numpy(), ref) and np.array_equal(got['x'].cpu().numpy().view(np.uint32),
                                                                             io_.to_x(ref).view(np.uint32))
      say('%-12s   host: tests/image_oracle.py (NumPy int64) on the same batch: %.2f s wall = %.0f x (b); its levels and x %s the '
          'device\'s' % ('', host_s, host_s / (float(np.median(ts['b'])) * 1e-6), 'EQUAL' if same else 'DIFFER FROM'))
    del src, x, got
  if '--no-png' not in sys.argv:
    png_lines(say)
  if out_path:
    with open(out_path, 'w') as f:
      f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
  main()
