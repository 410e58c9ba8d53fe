"""A pure-Python restatement of the zlib stream that the device PNG encoder writes (include/recattend.h, ra_png_deflate_*),
written from RFC 1950 / 1951 and the format's statement, not from the C++: the third implementation beside the kernels and
ra_png_deflate_host.  Slow and plain on purpose: one bit at a time, the length codes from the RFC's table.

  scanline  a filter-type byte 0, then the row (grey: W bytes, d = 1; colour: the FILE's R, G, B from a B, G, R array, d = 3)
  segment   one scanline: a fixed-Huffman block (BFINAL 0, BTYPE 01) of greedy run tokens at distance d, end-of-block, then an
            empty stored block (bits 0, 00, padding to the byte, 00 00 FF FF)
  stream    78 01, the segments, 03 00, the big-endian Adler-32 of all scanline bytes"""
import numpy as np

# RFC 1951 3.2.5: (code, extra bits, first length) of the length codes 257 .. 285
LENGTH_TABLE = [(257, 0, 3), (258, 0, 4), (259, 0, 5), (260, 0, 6), (261, 0, 7), (262, 0, 8), (263, 0, 9), (264, 0, 10),
                (265, 1, 11), (266, 1, 13), (267, 1, 15), (268, 1, 17), (269, 2, 19), (270, 2, 23), (271, 2, 27), (272, 2, 31),
                (273, 3, 35), (274, 3, 43), (275, 3, 51), (276, 3, 59), (277, 4, 67), (278, 4, 83), (279, 4, 99), (280, 4, 115),
                (281, 5, 131), (282, 5, 163), (283, 5, 195), (284, 5, 227), (285, 0, 258)]
DISTANCE_CODE = {1: 0, 3: 2}  # 3.2.5: distances 1 .. 4 are the codes 0 .. 3, no extra bits


class Bits(object):
  """Bits packed from the least significant bit of every byte on (3.1.1)."""

  def __init__(self):
    self.bits = []

  def value(self, v, n):
    """a field other than a Huffman code: least significant bit first"""
    self.bits += [(v >> k) & 1 for k in range(n)]

  def code(self, v, n):
    """a Huffman code: most significant bit first"""
    self.bits += [(v >> k) & 1 for k in range(n - 1, -1, -1)]

  def pad(self):
    self.bits += [0] * (-len(self.bits) % 8)

  def tobytes(self):
    assert len(self.bits) % 8 == 0
    b = np.array(self.bits, dtype=np.uint8).reshape(-1, 8)
    return bytes((b << np.arange(8, dtype=np.uint8)).sum(axis=1).astype(np.uint8).tolist())


def fixed_symbol(out, sym):
  """3.2.6: the fixed code of a literal / length symbol."""
  if sym <= 143:
    out.code(0b00110000 + sym, 8)
  elif sym <= 255:
    out.code(0b110010000 + (sym - 144), 9)
  elif sym <= 279:
    out.code(sym - 256, 7)
  else:
    out.code(0b11000000 + (sym - 280), 8)


def match(out, length, d):
  code, extra, first = [row for row in LENGTH_TABLE if row[2] <= length][-1]
  assert 3 <= length <= 258 and 0 <= length - first < (1 << extra)
  fixed_symbol(out, code)
  out.value(length - first, extra)
  out.code(DISTANCE_CODE[d], 5)


def tokens(seg, d):
  """The greedy left-to-right run code of one segment: [('lit', byte) | ('match', length)]."""
  n, i, out = len(seg), 0, []
  while i < n:
    L = 0
    if i >= d:
      while L < 258 and i + L < n and seg[i + L] == seg[i + L - d]:
        L += 1
    if L >= 3:
      out.append(('match', L))
      i += L
    else:
      out.append(('lit', seg[i]))
      i += 1
  return out


def segment(seg, d):
  out = Bits()
  out.value(0, 1)  # BFINAL
  out.value(1, 2)  # BTYPE = 01
  for kind, v in tokens(seg, d):
    if kind == 'lit':
      fixed_symbol(out, v)
    else:
      match(out, v, d)
  fixed_symbol(out, 256)
  out.value(0, 1)  # an empty stored block: BFINAL 0
  out.value(0, 2)  # BTYPE = 00
  out.pad()
  return out.tobytes() + b'\x00\x00\xff\xff'


def adler32(data):
  a, b = 1, 0
  for v in data:
    a = (a + v) % 65521
    b = (b + a) % 65521
  return (b << 16) | a


def scanlines(img):
  """img uint8 [H,W] or [H,W,3] (B, G, R) -> (list of H scanlines as lists of ints, d)"""
  img = np.asarray(img)
  if img.ndim == 3:
    rows, d = img[:, :, ::-1].reshape(img.shape[0], -1), 3
  else:
    rows, d = img, 1
  return [[0] + [int(v) for v in r] for r in rows], d


def stream(img):
  """The zlib stream of one image."""
  rows, d = scanlines(img)
  body = b''.join(segment(r, d) for r in rows)
  raw = [v for r in rows for v in r]
  return b'\x78\x01' + body + b'\x03\x00' + adler32(raw).to_bytes(4, 'big')


def segment_bound(n):
  return -(-9 * n // 8) + 7


def stream_bound(H, W, bpp):
  return 8 + H * segment_bound(1 + W * bpp)
