"""Inputs of the mixed-full-size tests (test_ragged.py, test_ragged_gpu.py): six images of six sizes per kernel, the three
layouts they are packed in, and the float64 references of every image ALONE — computed once and shared.

Layouts.  'packed': no padding, in the listed order — the images whose width is a multiple of 4 then start at offsets that
are not (16 x 128 at 1850), so they take the element loads; 'reversed': no padding, the batch in reverse order; 'aligned':
ra_ops.pack_ragged's layout, every image at a multiple of 4 elements, where the images with w % 4 == 0 take the wide loads.
The geometry table is in ascending order of offset, so a layout is a batch order: results come back in that order and
unpermute() puts them into the listed one."""
import functools

import numpy as np

import fg_eval_oracle as feo
import ins_eval_oracle as ieo
import labels_oracle as lo

# (h, w): exactly one 16 x 128 tile; one pixel over the tile in each direction with an odd width; several tiles; down-sizing
EVAL_SIZES = ((37, 50), (16, 128), (17, 129), (1, 4), (33, 256), (5, 7))
EVAL_T, EVAL_HS, EVAL_WS = 4, 8, 12
LABEL_SIZES = ((37, 50), (16, 128), (17, 129), (4, 6), (33, 256), (5, 7))
LABEL_H, LABEL_W, LABEL_T = 4, 6, 3
LABEL_SEED = 1200
LAYOUTS = ('packed', 'reversed', 'aligned')


def layout(name, n):
  """(batch order as indices into the listed images, alignment in elements)"""
  return {'packed': (list(range(n)), 1), 'reversed': (list(range(n))[::-1], 1), 'aligned': (list(range(n)), 4)}[name]


def geometry(sizes, align):
  """[B,3] int64 (offset, h, w) and the element count: what ra_ops.ragged_geometry returns, restated for the CPU tests."""
  geo, end = np.zeros((len(sizes), 3), np.int64), 0
  for b, (h, w) in enumerate(sizes):
    start = -(-end // align) * align
    geo[b] = (start, h, w)
    end = start + h * w
  return geo, end


def flatten(images, geo, total, dtype, fill=0):
  flat = np.full((total,), fill, dtype)
  for (off, h, w), img in zip(geo.tolist(), images):
    flat[off:off + h * w] = np.asarray(img, dtype).reshape(-1)
  return flat


def unpermute(order, a):
  """Rows of `a` (in batch order) back into the listed order."""
  out = np.empty_like(a)
  out[np.asarray(order)] = a
  return out


@functools.lru_cache(maxsize=None)
def ins_eval_image(i):
  """Image i as ins_eval_oracle.make_case makes the tuple (1, 4, 8, 12, h, w, 1100 + i): a temporary entry in a copy of CASES."""
  h, w = EVAL_SIZES[i]
  saved = ieo.CASES
  ieo.CASES = dict(saved, _ragged=(1, EVAL_T, EVAL_HS, EVAL_WS, h, w, 1100 + i))
  try:
    return ieo.make_case('_ragged')
  finally:
    ieo.CASES = saved


@functools.lru_cache(maxsize=None)
def ins_eval_values(i, morph):
  h, w = EVAL_SIZES[i]
  return ieo.values(ins_eval_image(i)['yc'], h, w, morph)


@functools.lru_cache(maxsize=None)
def ins_eval_reference(i, K, with_fg, morph):
  """(lo, hi, share, ties, inter, area_b) of image i alone."""
  c, v = ins_eval_image(i), ins_eval_values(i, morph)
  fg = c['fg'] if with_fg else None
  thr = ieo.THRESHOLDS[K]
  return ieo.conditions(v, c['gt_ids'], c['inst_id'], thr, fg) + ieo.counts(v, c['gt_ids'], c['inst_id'], thr, fg)


@functools.lru_cache(maxsize=None)
def sweep_image(i):
  """(src float32 [1,8,12], v64 [1,h,w], gt uint8 [1,h,w]) of image i."""
  h, w = EVAL_SIZES[i]
  rng = np.random.RandomState(1100 + i)
  src = feo.smooth_map(rng, 1, EVAL_HS, EVAL_WS)
  return src, feo.upsample(src, h, w), feo.disc_labels(rng, 1, h, w)


SWEEP_THRESHOLDS = [0.5, 0.0, 0.9, 0.2, 0.7, 0.1, 0.8, 0.3, 0.6, 0.4]


def sweep_band(i, delta):
  """(lo, hi, pixels inside the band per threshold [K]) of image i: each a (count_a, sum_ab, sum_b) triple with N = 1."""
  _, v64, gt = sweep_image(i)
  thr = SWEEP_THRESHOLDS
  lo_, hi_ = feo.sweep_counts(v64, gt, thr, +delta), feo.sweep_counts(v64, gt, thr, -delta)
  inside = np.array([int(((v64 > t - delta) & ~(v64 > t + delta)).sum()) for t in thr])
  return lo_, hi_, inside


@functools.lru_cache(maxsize=None)
def label_image(i, dataset):
  h, w = LABEL_SIZES[i]
  return lo.ellipse_ids(np.random.RandomState(LABEL_SEED + i), 1, h, w, 5, dataset)[0]


@functools.lru_cache(maxsize=None)
def label_reference(i, dataset):
  return lo.assemble(label_image(i, dataset)[None], LABEL_H, LABEL_W, LABEL_T, dataset)
