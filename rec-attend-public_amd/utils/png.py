"""8-bit greyscale PNG files on zlib + struct only (what cv2.imwrite(name, uint8 [H,W]) produces for the instance
masks of analysis.py:255-257; cv2 is not part of this stack).  One IHDR, one IDAT, one IEND chunk; filter type 0 on
every row.  `decode_gray8` reads exactly that subset back (tests, tools)."""
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
