"""The batches of MIXED sizes the ragged PNG encoder's tests run on (tests/test_png_ragged.py on the host entries,
tests/test_png_ragged_gpu.py on the device): M planes that share one geometry table, in three layouts, and the reference every
test compares with — the UNIFORM host entry (ops.png_deflate_host, pinned to zlib and to the Python restatements by
tests/test_png_device.py and tests/test_png_dynamic.py) of each image alone, computed once per (batch, kind, format).

  mixed   B = 8: w = 16 and 64 first (at 16-byte aligned offsets in every layout: the wide-load form), w = 1, w = 65, 258, 259 and
          517 (png_cases.WIDTHS: the chunk and match-length edges), h = 1, h = 17 (more than the 16 rows a compact / place
          workgroup takes) and 261 x 5 (a second scan trip of 256 rows).  Plane m holds png_cases.contents' m-th content of
          every image: zeros, ones, alternating, random (and equal_channels for colour).
  runs    png_cases.run_images — every match length and its extra bits — beside a 1 x 1 image; one plane."""
import functools

import numpy as np

import png_cases as pc
import ra_ops as ops

KINDS = ('grey', 'colour', 'float')
CODES = ('fixed', 'dynamic')
BATCHES = ('mixed', 'runs')
MIXED = ((2, 16), (3, 64), (7, 1), (3, 65), (2, 258), (17, 259), (1, 517), (261, 5))
# (name, align of ops.ragged_geometry, images laid out in reversed order)
LAYOUTS = (('packed', 1, False), ('align4', 4, False), ('align16-reversed', 16, True))


def _as_float(img):
  """The float plane whose quantisation (uint8)(v * 255.0f) is defined: k / 255 in float32."""
  return img.astype(np.float32) / np.float32(255.0)


def quantised(img):
  """The bytes the encoder makes of a float image (include/recattend.h: (uint8)(v * 255.0f) in float32)."""
  return (img * np.float32(255.0)).astype(np.uint8) if img.dtype == np.float32 else img


@functools.lru_cache(maxsize=None)
def planes(batch, kind):
  """[M][B] images: uint8 [h,w] (grey), uint8 [h,w,3] in B, G, R order (colour) or float32 [h,w] (float)."""
  base = 'colour' if kind == 'colour' else 'grey'
  if batch == 'runs':
    run = [img for _, k, img in pc.run_images() if k == base][0]
    out = [[run, np.full((1, 1) + run.shape[2:], 7, np.uint8)]]
  else:
    per_image = [[img for _, img in pc.contents(base, h, w, 1000 * w + h)] for h, w in MIXED]
    out = [[c[m] for c in per_image] for m in range(len(per_image[0]))]
  return [[_as_float(i) for i in p] for p in out] if kind == 'float' else out


def scanlines(img):
  """What zlib.decompress of the image's stream returns: per row a filter-type byte 0 and the file's bytes (R, G, B)."""
  img = quantised(np.asarray(img))
  rows = (img[:, :, ::-1] if img.ndim == 3 else img).reshape(img.shape[0], -1)
  return np.concatenate([np.zeros((img.shape[0], 1), np.uint8), rows], axis=1).tobytes()


@functools.lru_cache(maxsize=None)
def reference(batch, kind, code):
  """[M][B] (stream, adler): the uniform host entry on each image alone."""
  out = []
  for p in planes(batch, kind):
    row = []
    for img in p:
      z, a = ops.png_deflate_host(img[None], code=code)
      row.append((z[0], int(a[0])))
    out.append(row)
  return out


def layout(batch, kind, name):
  """(src [M,P] or [M,P,3] NumPy, geometry [B,3], order): table entry b of the layout is image order[b] of planes(batch, kind)."""
  _, align, reverse = [l for l in LAYOUTS if l[0] == name][0]
  ps = planes(batch, kind)
  order = list(range(len(ps[0])))[::-1] if reverse else list(range(len(ps[0])))
  geo, total = ops.ragged_geometry([ps[0][j].shape[:2] for j in order], align)
  src = np.zeros((len(ps), total) + ps[0][0].shape[2:], ps[0][0].dtype)
  for m, p in enumerate(ps):
    for (off, h, w), j in zip(geo.tolist(), order):
      src[m, off:off + h * w] = p[j].reshape((h * w,) + p[j].shape[2:])
  return src, geo, order


def expected(batch, kind, code, order, plane_index=None):
  """The (stream, adler) list of a ragged call in stream order: plane-major, the images in the layout's order."""
  ref = reference(batch, kind, code)
  ks = range(len(ref)) if plane_index is None else plane_index
  return [ref[k][j] for k in ks for j in order]
