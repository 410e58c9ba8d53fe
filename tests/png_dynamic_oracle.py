"""A pure-Python restatement of the device PNG encoder's "dynamic" stream (include/recattend.h, ra_png_deflate_dyn_*), written
from RFC 1950 / 1951 and the format's statement, not from the C++: the third implementation beside the kernels and
ra_png_deflate_dyn_host.  Slow and plain on purpose: one bit at a time, lists and dictionaries.  The scanlines, the greedy token
walk, the length table and the bit packer are those of tests/png_deflate_oracle.py (the two formats share them by definition).

  stream   78 01; one block BFINAL 1, BTYPE 10: HLIT, HDIST, HCLEN, the code-length code's lengths, the run-length coded length
           sequence, the tokens of all rows back to back, end-of-block; zero bits to the byte; the big-endian Adler-32
  lengths  two-queue Huffman over the used symbols sorted by (count, symbol), a leaf before an internal node on a tie; while the
           deepest leaf is deeper than the limit every count becomes (c + 1) >> 1 and the tree is rebuilt"""
from collections import deque

import numpy as np

import png_deflate_oracle as fixed

CODE_LENGTH_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)  # RFC 1951 3.2.7


def tree_depths(counts):
  """{symbol: depth of its leaf} of the two-queue Huffman tree over the symbols with a count above 0 (at least two)."""
  leaves = deque(sorted((c, s) for s, c in enumerate(counts) if c > 0))
  inner = deque()  # (weight, [symbols below]) in the order they are made
  depth = {s: 0 for _, s in leaves}

  def smallest():
    if leaves and (not inner or leaves[0][0] <= inner[0][0]):
      c, s = leaves.popleft()
      return c, [s]
    return inner.popleft()

  while len(leaves) + len(inner) > 1:
    (ca, sa), (cb, sb) = smallest(), smallest()
    for s in sa + sb:
      depth[s] += 1
    inner.append((ca + cb, sa + sb))
  return depth


def unlimited_depth(counts):
  return max(tree_depths(counts).values())


def limited_lengths(counts, limit):
  """The rule: a list of len(counts) code lengths, none above limit."""
  counts = [int(c) for c in counts]
  used = [s for s, c in enumerate(counts) if c > 0]
  out = [0] * len(counts)
  if len(used) == 1:
    out[used[0]] = 1
  if len(used) < 2:
    return out
  while True:
    depth = tree_depths(counts)
    if max(depth.values()) <= limit:
      break
    counts = [(c + 1) >> 1 if c > 0 else 0 for c in counts]
  for s, k in depth.items():
    out[s] = k
  return out


def canonical(lengths):
  """RFC 1951 3.2.2: {symbol: (code, length)} of the used symbols."""
  codes, code = {}, 0
  for bits in range(1, max(lengths) + 1):
    for s, k in enumerate(lengths):
      if k == bits:
        codes[s] = (code, bits)
        code += 1
    code <<= 1
  return codes


def run_lengths(seq):
  """The length sequence as [(code-length symbol, extra value, extra bits)]: zero runs as 18s, then a 17, then single zeros."""
  out, i = [], 0
  while i < len(seq):
    if seq[i] != 0:
      out.append((seq[i], 0, 0))
      i += 1
      continue
    run = 0
    while i < len(seq) and seq[i] == 0:
      run, i = run + 1, i + 1
    while run >= 11:
      take = min(run, 138)
      out.append((18, take - 11, 7))
      run -= take
    if run >= 3:
      out.append((17, run - 3, 3))
      run = 0
    out += [(0, 0, 0)] * run
  return out


def length_symbol(length):
  code, extra, first = [row for row in fixed.LENGTH_TABLE if row[2] <= length][-1]
  return code, length - first, extra


def histogram(rows, d):
  counts = [0] * 286
  for r in rows:
    for kind, v in fixed.tokens(r, d):
      counts[v if kind == 'lit' else length_symbol(v)[0]] += 1
  counts[256] += 1
  return counts


def stream_bits(img):
  """(the Bits of everything before the Adler-32, [the bit place of every row's first token], the rows, d)."""
  rows, d = fixed.scanlines(img)
  lengths = limited_lengths(histogram(rows, d), 15)
  codes = canonical(lengths)
  n_lit = max(s for s, k in enumerate(lengths) if k) + 1
  dist = [1] if d == 1 else [0, 0, 1]
  runs = run_lengths(lengths[:n_lit] + dist)
  cl_counts = [0] * 19
  for sym, _, _ in runs:
    cl_counts[sym] += 1
  cl_lengths = limited_lengths(cl_counts, 7)
  cl_codes = canonical(cl_lengths)
  n_cl = max(4, max(k for k, sym in enumerate(CODE_LENGTH_ORDER) if cl_lengths[sym]) + 1)
  out = fixed.Bits()
  out.value(0x78, 8)
  out.value(0x01, 8)
  out.value(1, 1)  # BFINAL
  out.value(2, 2)  # BTYPE = 10
  out.value(n_lit - 257, 5)
  out.value(len(dist) - 1, 5)
  out.value(n_cl - 4, 4)
  for sym in CODE_LENGTH_ORDER[:n_cl]:
    out.value(cl_lengths[sym], 3)
  for sym, extra, nbits in runs:
    out.code(*cl_codes[sym])
    out.value(extra, nbits)
  starts = []
  for r in rows:
    starts.append(len(out.bits))
    for kind, v in fixed.tokens(r, d):
      if kind == 'lit':
        out.code(*codes[v])
      else:
        sym, extra, nbits = length_symbol(v)
        out.code(*codes[sym])
        out.value(extra, nbits)
        out.code(0, 1)  # the one distance code, length 1
  starts.append(len(out.bits))  # end-of-block
  out.code(*codes[256])
  return out, starts, rows, d


def stream(img):
  """The zlib stream of one image."""
  out, _, rows, _ = stream_bits(img)
  out.pad()
  return out.tobytes() + fixed.adler32([v for r in rows for v in r]).to_bytes(4, 'big')


def row_places(img):
  """The bit place, from the stream's first byte on, of every row's first token and of the end-of-block code."""
  return stream_bits(img)[1]


def stream_bound(H, W, bpp):
  return 270 + -(-15 * (1 + W * bpp) * H // 8)


def fibonacci(k):
  """[1, 1, 2, 3, 5, ...], k numbers."""
  out = [1, 1]
  while len(out) < k:
    out.append(out[-1] + out[-2])
  return out[:k]


def forced_limit_image():
  """uint8 [1991, 61]: the byte values 1 .. 24 with Fibonacci counts 1, 1, 2, ... 46368 (121392 pixels, value 24 once more for
  each of the 59 pixels that fill the last row), shuffled with a fixed seed.  The unlimited Huffman tree of its literal
  histogram is deeper than 15, so the limiter's halving round runs through the whole path."""
  px = np.concatenate([np.full((c,), v + 1, np.uint8) for v, c in enumerate(fibonacci(24))])
  px = np.concatenate([px, np.full((-px.size % 61,), 24, np.uint8)])
  np.random.RandomState(2024).shuffle(px)
  return px.reshape(-1, 61)
