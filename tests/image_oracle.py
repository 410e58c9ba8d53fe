"""The image stage in NumPy, written from the definition in include/recattend.h (the section of csrc/ra_image.hip), not from
the kernel: the tables and the fixed-point bicubic resize of cv2.resize(..., INTER_CUBIC) on 8-bit images
(ins_seg_assembler.py:116) as that header restates them, and a PNG encoder for the tests of utils/png.py's colour reader
that picks the filter type of every row, on zlib + struct."""
import struct
import zlib

import numpy as np

COEF_BITS = 11
SHAPES = [((16, 32), (4, 8)), ((37, 53), (16, 24)), ((9, 7), (20, 13)), ((1, 5), (3, 4)), ((2, 3), (5, 2)), ((3, 3), (7, 7)),
          ((70, 130), (40, 100))]  # (Hs, Ws) -> (H, W): the issue's list but the one KITTI-sized image
KITTI_SHAPE = ((375, 1242), (128, 448))


def cubic_table(S, D):
  """One axis, source length S -> destination length D: (ofs int32 [D], coef int16 [D,4])."""
  f32 = np.float32
  d = np.arange(D, dtype=np.float64)
  f = ((d + 0.5) * (float(S) / float(D)) - 0.5).astype(f32)
  s = np.floor(f)
  t = (f - s).astype(f32)
  A = f32(-0.75)
  one, two, three = f32(1), f32(2), f32(3)
  t1, u = t + one, one - t
  c0 = ((A * t1 - f32(5) * A) * t1 + f32(8) * A) * t1 - f32(4) * A
  c1 = ((A + two) * t - (A + three)) * t * t + one
  c2 = ((A + two) * u - (A + three)) * u * u + one
  c3 = one - c0 - c1 - c2
  c = np.stack([c0, c1, c2, c3], axis=1)
  assert c.dtype == np.float32 and t.dtype == np.float32
  q = np.rint(c * f32(1 << COEF_BITS)).astype(np.int16)  # np.rint: half to even
  return s.astype(np.int32), q


def _taps(S, D):
  ofs, q = cubic_table(S, D)
  idx = np.clip(ofs[:, None] - 1 + np.arange(4)[None, :], 0, S - 1)
  return idx, q.astype(np.int64)


def resize_cubic_unclipped(img, H, W):
  """int64 [..., H, W, C]: v of the definition before the rounding shift and the clamp (v / 2^22 is the float value)."""
  img = np.asarray(img)
  assert img.dtype == np.uint8 and img.ndim >= 3
  Hs, Ws = img.shape[-3], img.shape[-2]
  iy, qy = _taps(Hs, H)
  ix, qx = _taps(Ws, W)
  src = img.astype(np.int64)
  h = (src[..., :, ix, :] * qx[:, :, None]).sum(axis=-2)         # [..., Hs, W, C]
  return (h[..., iy, :, :] * qy[:, :, None, None]).sum(axis=-3)  # [..., H, W, C]


def resize_cubic_u8(img, H, W):
  """img uint8 [..., Hs, Ws, C] -> uint8 [..., H, W, C]."""
  v = resize_cubic_unclipped(img, H, W)
  assert np.abs(v).max() < 1 << 31  # the int32 of the definition does not overflow
  return np.clip((v + (1 << (2 * COEF_BITS - 1))) >> (2 * COEF_BITS), 0, 255).astype(np.uint8)


def to_x(u8):
  """ins_seg_dataset.py:149"""
  return u8.astype(np.float32) / 255


def checkerboard(H=24, W=36, square=3):
  r, c = np.arange(H)[:, None] // square, np.arange(W)[None, :] // square
  return np.repeat((((r + c) & 1) * 255).astype(np.uint8)[:, :, None], 3, axis=2)


# ---- PNG
def _chunk(tag, data):
  return struct.pack('>I', len(data)) + tag + data + struct.pack('>I', zlib.crc32(tag + data) & 0xffffffff)


def filter_rows(rows, bpp, filters):
  """rows uint8 [H,stride] -> the filtered scanlines (PNG specification 9.2), one filter-type byte in front of each, byte by
  byte; filters: one type for all rows or a sequence that is cycled."""
  rows = np.asarray(rows).astype(int)
  H, stride = rows.shape
  filters = [filters] * H if np.isscalar(filters) else [filters[r % len(filters)] for r in range(H)]
  raw = bytearray()
  for r in range(H):
    ft = filters[r]
    raw.append(ft)
    for i in range(stride):
      a = rows[r, i - bpp] if i >= bpp else 0
      b = rows[r - 1, i] if r > 0 else 0
      c = rows[r - 1, i - bpp] if (r > 0 and i >= bpp) else 0
      if ft == 0:
        pred = 0
      elif ft == 1:
        pred = a
      elif ft == 2:
        pred = b
      elif ft == 3:
        pred = (a + b) // 2
      else:
        p = a + b - c
        pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
        pred = a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)
      raw.append((rows[r, i] - pred) % 256)
  return bytes(raw)


def encode_png(img, colour_type, depth=8, filters=0, palette=None, idat_split=1, interlace=0):
  """A PNG file of img: [H,W,3] RGB (colour type 2), [H,W,4] RGBA (6), [H,W] palette indices (3, depth 1 | 2 | 4 | 8, palette
  uint8 [n,3] RGB) or [H,W] grey (0); 8-bit samples, or 16-bit ones (depth 16) for the refusals.  `interlace` only sets the
  header's byte."""
  img = np.asarray(img)
  H, W = img.shape[:2]
  channels = {0: 1, 2: 3, 3: 1, 6: 4}[colour_type]
  if depth == 16:
    rows = np.frombuffer(np.ascontiguousarray(img, dtype='>u2').tobytes(), np.uint8).reshape(H, -1)
  elif depth == 8:
    rows = np.ascontiguousarray(img, dtype=np.uint8).reshape(H, W * channels)
  else:  # samples packed into bytes, the leftmost in the high bits, rows padded to a byte
    per = 8 // depth
    padded = np.zeros((H, -(-W // per) * per), np.uint8)
    padded[:, :W] = img
    rows = np.zeros((H, padded.shape[1] // per), np.uint8)
    for k in range(per):
      rows |= padded[:, k::per] << (8 - depth * (k + 1))
  bpp = max(1, channels * depth // 8)
  z = zlib.compress(filter_rows(rows, bpp, filters))
  cuts = [len(z) * k // idat_split for k in range(idat_split + 1)]
  out = b'\x89PNG\r\n\x1a\n' + _chunk(b'IHDR', struct.pack('>IIBBBBB', W, H, depth, colour_type, 0, 0, interlace))
  if palette is not None:
    out += _chunk(b'PLTE', np.ascontiguousarray(palette, dtype=np.uint8).tobytes())
  for k in range(idat_split):
    out += _chunk(b'IDAT', z[cuts[k]:cuts[k + 1]])
  return out + _chunk(b'IEND', b'')
