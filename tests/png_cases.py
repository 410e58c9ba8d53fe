"""The images the PNG deflate tests run on (tests/test_png_device.py on the host entry, tests/test_png_device_gpu.py on the
device): the sizes and contents at which the stream format can go wrong.  Every image is uint8 [H,W] (grey, run distance 1) or
[H,W,3] in B, G, R memory order (colour, run distance 3); all images of one group share a shape, so a group is one batched call."""
import numpy as np

WIDTHS = (1, 2, 3, 4, 5, 63, 64, 65, 257, 258, 259, 260, 261, 262, 517, 1031)
HEIGHTS = (1, 2, 7)
KINDS = ('grey', 'colour')


def _shape(kind, H, W):
  return (H, W) if kind == 'grey' else (H, W, 3)


def alternating(kind, H, W):
  """No byte equals the one d before it: two values, both coded with 9 bits, alternating per pixel.  The stream is as long
  as the format lets it get."""
  px = np.where((np.arange(W)[None, :] + np.arange(H)[:, None]) % 2 == 0, 200, 255).astype(np.uint8)
  return px if kind == 'grey' else np.repeat(px[:, :, None], 3, axis=2)


def equal_channels(seed, H, W):
  """Colour pixels equal in all three channels, in short pixel runs: bytes that repeat at distance 1 AND at distance 3."""
  rs = np.random.RandomState(seed)
  px = np.repeat(rs.randint(0, 256, size=(H, W)), rs.randint(1, 5), axis=1)[:, :W].astype(np.uint8)
  return np.ascontiguousarray(np.repeat(px[:, :, None], 3, axis=2))


def contents(kind, H, W, seed):
  """[(name, image)] of one shape."""
  rs = np.random.RandomState(seed)
  out = [('zeros', np.zeros(_shape(kind, H, W), np.uint8)), ('ones', np.full(_shape(kind, H, W), 255, np.uint8)),
         ('alternating', alternating(kind, H, W)), ('random', rs.randint(0, 256, size=_shape(kind, H, W)).astype(np.uint8))]
  if kind == 'colour':
    out.append(('equal_channels', equal_channels(seed + 1, H, W)))
  return out


def grid():
  """[(id, kind, W, [(name, image)])]: per kind and width, every height and content."""
  out = []
  for kind in KINDS:
    for W in WIDTHS:
      imgs = []
      for H in HEIGHTS:
        imgs += [('%s-H%d' % (name, H), img) for name, img in contents(kind, H, W, 1000 * W + H)]
      out.append(('%s-W%d' % (kind, W), kind, W, imgs))
  return out


RUN_ROW_BYTES = 642  # = 3 * 214: the same byte rows serve as a grey image of W = 642 and a colour image of W = 214


def run_rows(d):
  """uint8 [150, RUN_ROW_BYTES]: the FILE's bytes of 150 rows.  Row k (R = k + 1) holds, at distance d, a stretch of exactly R
  positions that equal the byte d before them, one that does not, a stretch of 301 - R, and none from there on: the stretches
  1 .. 300 all occur, so every length code 257 .. 285 with all its extra bits, and 258 followed by remainders 0, 1, 2 and 3."""
  rows = np.zeros((150, RUN_ROW_BYTES), np.uint8)
  for k in range(150):
    R = k + 1
    plan = [False] * d + [True] * R + [False] + [True] * (301 - R)
    plan += [False] * (RUN_ROW_BYTES - len(plan))
    seg = [0]  # the filter byte in front
    for i in range(1, RUN_ROW_BYTES + 1):
      before = seg[i - d] if i >= d else (3 * R + i) % 256
      seg.append(before if plan[i - 1] and i >= d else (before + 1 + (7 * i + R) % 200) % 256)
    rows[k] = seg[1:]
  return rows


def run_images():
  """[(id, kind, image)]: run_rows as a grey image and, with the channels put into memory order, as a colour image."""
  colour = run_rows(3).reshape(150, RUN_ROW_BYTES // 3, 3)[:, :, ::-1]
  return [('runs-grey', 'grey', run_rows(1)), ('runs-colour', 'colour', np.ascontiguousarray(colour))]


def white_row():
  """One colour row of 1860 white pixels: 5581 scanline bytes of 255 (and the filter byte), more than the 5552 zlib lets
  itself sum between two reductions of its Adler-32 accumulators."""
  return np.full((1, 1860, 3), 255, np.uint8)


def expected_stretches(rows, d):
  """The lengths of all maximal stretches of positions i >= d with seg[i] == seg[i-d] in the scanlines of `rows` (file bytes)."""
  found = set()
  for r in rows:
    seg = np.concatenate([[0], r]).astype(np.int64)
    eq = np.concatenate([[False] * d, seg[d:] == seg[:-d], [False]])
    edges = np.flatnonzero(np.diff(np.concatenate([[0], eq.astype(np.int8)])))
    found.update(int(b - a) for a, b in zip(edges[0::2], edges[1::2]))
  return found
