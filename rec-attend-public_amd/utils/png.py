"""8-bit greyscale PNG files on zlib + struct only (what cv2.imwrite(name, uint8 [H,W]) produces for the instance
masks of analysis.py:255-257; cv2 is not part of this stack).  One IHDR, one IDAT, one IEND chunk; filter type 0 on
every row.  `decode_gray8` reads exactly that subset back (tests, tools).

`decode_gray16` / `read_gray16` read 16-bit greyscale files (*_gtFine_instanceIds.png of the Cityscapes ground truth) as
other encoders write them: any number of IDAT chunks and all five row filters of the PNG specification (section 9).  A
file whose rows use None, Sub and Up is undone a row at a time (tens of ms for 1024 x 2048); one that holds Average or Paeth
rows is undone by anti-diagonals, about a second for that size in NumPy, which a compiled loop would cut further (not built)."""
import struct
import zlib

import numpy as np

SIGNATURE = b'\x89PNG\r\n\x1a\n'


def _chunk(tag, data):
  return struct.pack('>I', len(data)) + tag + data + struct.pack('>I', zlib.crc32(tag + data) & 0xffffffff)


def encode_gray8(img, level=6):
  """img: uint8 [H,W] -> the bytes of a PNG file (colour type 0, bit depth 8, no interlace)."""
  img = np.ascontiguousarray(img)
  if img.dtype != np.uint8 or img.ndim != 2 or img.shape[0] < 1 or img.shape[1] < 1:
    raise ValueError('encode_gray8 needs a uint8 [H,W] array, got %s %s' % (img.dtype, img.shape))
  H, W = img.shape
  rows = np.zeros((H, W + 1), dtype=np.uint8)  # a filter-type byte (0 = None) in front of every row
  rows[:, 1:] = img
  ihdr = struct.pack('>IIBBBBB', W, H, 8, 0, 0, 0, 0)
  return SIGNATURE + _chunk(b'IHDR', ihdr) + _chunk(b'IDAT', zlib.compress(rows.tobytes(), level)) + _chunk(b'IEND', b'')


def write_gray8(path, img, level=6):
  with open(path, 'wb') as f:
    f.write(encode_gray8(img, level))


def iter_chunks(data):
  """(tag, payload, stored crc) of every chunk; raises ValueError on a bad signature or a truncated file."""
  if data[:8] != SIGNATURE:
    raise ValueError('not a PNG file')
  pos = 8
  while pos < len(data):
    if pos + 8 > len(data):
      raise ValueError('truncated PNG chunk header')
    n, = struct.unpack('>I', data[pos:pos + 4])
    tag = data[pos + 4:pos + 8]
    if pos + 12 + n > len(data):
      raise ValueError('truncated PNG chunk')
    crc, = struct.unpack('>I', data[pos + 8 + n:pos + 12 + n])
    yield tag, data[pos + 8:pos + 8 + n], crc
    pos += 12 + n


def decode_gray8(data):
  """The inverse of encode_gray8 (8-bit greyscale, filter 0 only, CRCs checked) -> uint8 [H,W]."""
  shape, idat = None, b''
  for tag, payload, crc in iter_chunks(data):
    if zlib.crc32(tag + payload) & 0xffffffff != crc:
      raise ValueError('bad CRC in chunk %r' % tag)
    if tag == b'IHDR':
      W, H, depth, colour, comp, flt, lace = struct.unpack('>IIBBBBB', payload)
      if (depth, colour, comp, flt, lace) != (8, 0, 0, 0, 0):
        raise ValueError('only 8-bit greyscale, non-interlaced PNG files are read here')
      shape = (H, W)
    elif tag == b'IDAT':
      idat += payload
  if shape is None:
    raise ValueError('no IHDR chunk')
  rows = np.frombuffer(zlib.decompress(idat), dtype=np.uint8).reshape(shape[0], shape[1] + 1)
  if rows[:, 0].any():
    raise ValueError('only filter type 0 is read here')
  return rows[:, 1:].copy()


def read_gray8(path):
  with open(path, 'rb') as f:
    return decode_gray8(f.read())


def _unfilter_rows(raw, H, stride, bpp):
  """_unfilter for files whose rows use the filters None, Sub and Up only: one NumPy expression per row."""
  out = np.zeros((H, stride), dtype=np.uint8)
  prev = np.zeros(stride, dtype=np.int64)
  for r in range(H):
    ft, v = raw[r, 0], raw[r, 1:].astype(np.int64)
    if ft == 2:  # Up
      v = (v + prev) & 255
    elif ft == 1:  # Sub: a running sum (mod 256) along each of the bpp byte lanes
      for k in range(bpp):
        v[k::bpp] = np.cumsum(v[k::bpp]) & 255
    out[r] = prev = v
  return out


def _unfilter_diagonals(raw, H, stride, bpp):
  """_unfilter for files that hold Average or Paeth rows.  A byte of those needs the reconstructed bytes to its left, above
  it and above left, so neither a row nor a column can be undone at once; the pixels of one anti-diagonal (row + column
  constant) need only the two diagonals before them.  Walk the H + W - 1 diagonals, every one a NumPy expression over its
  pixels with the predictor chosen by the row's filter type: a 1024 x 2048 16-bit image takes 3071 steps, not 4 M."""
  W = stride // bpp
  ft = raw[:, 0].astype(np.int64)[:, None]
  x = raw[:, 1:].astype(np.int64).reshape(H, W, bpp)
  out = np.zeros((H + 1, W + 1, bpp), dtype=np.int64)  # a zero row above and a zero column to the left (9.2)
  for d in range(H + W - 1):
    r = np.arange(max(0, d - W + 1), min(H - 1, d) + 1)
    c = d - r
    a, b, cc = out[r + 1, c], out[r, c + 1], out[r, c]  # left, above, above left
    pa, pb, pc = np.abs(b - cc), np.abs(a - cc), np.abs(a + b - 2 * cc)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, cc))
    f = ft[r]
    pred = np.where(f == 0, 0, np.where(f == 1, a, np.where(f == 2, b, np.where(f == 3, (a + b) >> 1, paeth))))
    out[r + 1, c + 1] = (x[r, c] + pred) & 255
  return out[1:, 1:].reshape(H, stride).astype(np.uint8)


def _unfilter(raw, H, stride, bpp):
  """The scanlines of a non-interlaced image with the filter of every row undone (PNG specification, 9.2): raw holds H rows
  of one filter-type byte + stride bytes, bpp = bytes per complete pixel.  -> uint8 [H, stride]."""
  if len(raw) != H * (stride + 1):
    raise ValueError('PNG image data has %d bytes, %d expected' % (len(raw), H * (stride + 1)))
  raw = np.frombuffer(raw, dtype=np.uint8).reshape(H, stride + 1)
  if raw[:, 0].max() > 4:
    r = int(np.argmax(raw[:, 0] > 4))
    raise ValueError('PNG row %d has filter type %d' % (r, raw[r, 0]))
  return (_unfilter_diagonals if (raw[:, 0] >= 3).any() else _unfilter_rows)(raw, H, stride, bpp)


def decode_gray16(data):
  """16-bit greyscale, non-interlaced PNG (colour type 0, bit depth 16; all five row filters; CRCs checked) -> uint16 [H,W]."""
  shape, idat = None, b''
  for tag, payload, crc in iter_chunks(data):
    if zlib.crc32(tag + payload) & 0xffffffff != crc:
      raise ValueError('bad CRC in chunk %r' % tag)
    if tag == b'IHDR':
      W, H, depth, colour, comp, flt, lace = struct.unpack('>IIBBBBB', payload)
      if (depth, colour, comp, flt, lace) != (16, 0, 0, 0, 0):
        raise ValueError('only 16-bit greyscale, non-interlaced PNG files are read here (bit depth %d, colour type %d, '
                         'interlace %d)' % (depth, colour, lace))
      shape = (H, W)
    elif tag == b'IDAT':
      idat += payload
  if shape is None:
    raise ValueError('no IHDR chunk')
  H, W = shape
  try:
    raw = zlib.decompress(idat)
  except zlib.error as e:
    raise ValueError('PNG image data does not inflate: %s' % e)
  rows = _unfilter(raw, H, 2 * W, 2)
  return (rows[:, 0::2].astype(np.uint16) << 8) | rows[:, 1::2]  # big-endian samples


def read_gray16(path):
  with open(path, 'rb') as f:
    return decode_gray16(f.read())
