"""Seeded inputs of the toolkit fixtures (tests/golden/toolkit_*.npz): the scenes that oracle/toolkit_fixtures.py runs through
the reference's own evaluation programs, and the packing of those scenes into the fixture files.  The generators are called
twice: by the recipe, which records what the reference's programs computed on them, and by tests/test_toolkit_fixtures.py,
which checks that they still give the committed inputs bit for bit.  Nothing here reads the reference.

  instance level  a scene is what ap_oracle.scene returns: gt_ids int32 [B,H,W], y float32 [B,T,H,W] of 0 / 1, label_id int32
                  [B,T] (-1 = slot not written), conf float32 [B,T], names;
  pixel level     a scene is (pred uint8, gt_labels uint8, gt_ids int32), each [B,H,W];
  orientation     a scene is an id image uint8 [B,H,W]: every id != 0 is one instance."""
import json

import numpy as np

import ap_oracle as ao
import labels_oracle as lo
import pixel_oracle as po

ORI_GUARD = 1e-6        # tests/test_labels_gpu.py's guard around the floor of the orientation value
EDGE_EXCLUDED_CAP = 0.05  # at most this share of the edge masks' foreground may lie inside the guard

EVALUATED = [l for _, l in ao.INST_LABELS]
STUFF = [7, 8, 11, 21, 23]
VOID = [0, 1, 3, 4]

# name: (kind, seed, B, H, W, T, instances per image).  A seed must not leave a class with ground truth and predictions but
# without a single example (every prediction ignored, no instance matched): the toolkit itself ends in an IndexError there
# (analysis.cityscapes_ap says what the product does).  The recipe runs the oracle first, which fails in the same way.
INSTANCE_SCENES = {
    'legacy0': ('legacy', 0, 3, 96, 160, 8, 0),           # ap_oracle.scene(0): hand-placed, takes every branch
    'random1': ('random', 1, 3, 96, 160, 20, 9),
    'random2': ('random', 2, 3, 96, 160, 20, 9),
    'random3': ('random', 13, 3, 96, 160, 20, 12),
    'random4': ('random', 4, 3, 96, 160, 20, 6),
    'odd37x53': ('random', 15, 3, 37, 53, 16, 5),          # H * W = 1961: no multiple of 4, the tail of the 16-byte loads
    'many40': ('random', 6, 2, 64, 96, 40, 8),            # 40 predictions on an image: two launches of the overlap kernel
}
# name: (seed, B, H, W)
PIXEL_SCENES = {
    'p48x80': (11, 3, 48, 80),
    'p37x53': (12, 2, 37, 53),
    'special48x80': (13, 3, 48, 80),   # image 1 predicts label 0 everywhere, image 2 holds an instance of a single pixel
    'zero37x53': (14, 1, 37, 53),      # label 0 everywhere and nothing else: every score is 0 or NaN
}
# name: (seed, B, H, W); seed None = the hand-made edge masks
ORIENTATION_SCENES = {
    'ellipses21': (21, 3, 60, 90),
    'ellipses22': (22, 3, 60, 90),
    'edges': (None, 1, 21, 33),
}
EDGE_IDS = {1: 'one pixel', 2: 'horizontal line', 3: 'vertical line', 4: 'square', 5: 'one pixel in the corner (0, 0)'}


# ---- instance level
def _shape_mask(rng, H, W, hmin, hmax, wmin, wmax):
  """A random rectangle or ellipse of about h x w pixels, clipped to the image."""
  h, w = rng.randint(hmin, hmax + 1), rng.randint(wmin, wmax + 1)
  r, c = rng.randint(0, H - h + 1), rng.randint(0, W - w + 1)
  m = np.zeros((H, W), bool)
  if rng.rand() < 0.5:
    m[r:r + h, c:c + w] = True
  else:
    rr, cc = np.mgrid[0:H, 0:W]
    m[((rr - (r + (h - 1) / 2.0)) / (h / 2.0)) ** 2 + ((cc - (c + (w - 1) / 2.0)) / (w / 2.0)) ** 2 <= 1.0] = True
  return m


def _jitter(rng, m, amount):
  """The mask moved by up to `amount` pixels each way (what leaves the image is lost), at times with a side cut off."""
  H, W = m.shape
  dy, dx = rng.randint(-amount, amount + 1), rng.randint(-amount, amount + 1)
  out = np.zeros_like(m)
  out[max(dy, 0):H + min(dy, 0), max(dx, 0):W + min(dx, 0)] = m[max(-dy, 0):H + min(-dy, 0), max(-dx, 0):W + min(-dx, 0)]
  if rng.rand() < 0.4:
    rows = np.where(out.any(axis=1))[0]
    if rows.size > 3:
      out[rows[0]:rows[0] + rng.randint(1, max(2, rows.size // 4))] = False
  return out


def _random_instance_scene(seed, B, H, W, T, n_inst):
  rng = np.random.RandomState(seed)
  gt = np.zeros((B, H, W), np.int32)
  y = np.zeros((B, T, H, W), np.float32)
  lab = np.full((B, T), -1, np.int32)
  conf = np.zeros((B, T), np.float32)
  hmin, hmax, wmin, wmax = max(4, H // 6), max(6, H // 2), max(4, W // 8), max(6, W // 3)
  for b in range(B):
    img = gt[b]
    cuts = np.sort(rng.randint(1, H - 1, 2))
    img[:cuts[0]], img[cuts[0]:cuts[1]], img[cuts[1]:] = rng.choice(STUFF, 3)
    v0, v1 = H - max(3, H // 8), W // 4 + rng.randint(0, W // 4)
    img[v0:, :v1] = rng.choice(VOID)                        # a void band along part of the lower edge
    absent = int(rng.choice(EVALUATED)) if b == B - 1 else None  # the last image: a class that is predicted and has no instance
    allowed = [l for l in EVALUATED if l != absent]
    for k in range(n_inst):
      img[_shape_mask(rng, H, W, hmin, hmax, wmin, wmax)] = int(rng.choice(allowed)) * 1000 + k
    img[_shape_mask(rng, H, W, 5, 7, 6, 9)] = int(rng.choice(allowed)) * 1000 + n_inst        # below 100 pixels
    group_label = int(rng.choice(allowed))
    img[_shape_mask(rng, H, W, hmin, hmax, wmin, wmax)] = group_label                         # a group region
    img[_shape_mask(rng, H, W, hmin, hmax // 2 + 1, wmin, wmax // 2 + 1)] = int(rng.choice([29, 30])) * 1000 + n_inst + 1
    # painted last, so that the counts hold: an instance of exactly 100 pixels (the minimum region size) and one of 99
    r, c = rng.randint(0, H - 10 + 1), rng.randint(0, W - 20 + 1)
    id100, id99 = int(rng.choice(allowed)) * 1000 + n_inst + 2, int(rng.choice(allowed)) * 1000 + n_inst + 3
    img[r:r + 10, c:c + 10] = id100
    while True:
      r2, c2 = rng.randint(0, H - 9 + 1), rng.randint(0, W - 11 + 1)
      if r2 + 9 <= r or r2 >= r + 10 or c2 + 11 <= c or c2 >= c + 10:
        break
    img[r2:r2 + 9, c2:c2 + 11] = id99
    inst = [int(i) for i in np.unique(img) if i >= 1000 and i // 1000 in EVALUATED and i not in (id100, id99)]
    preds = []                                               # (mask, label), the special ones first
    preds.append((np.zeros((H, W), bool), int(rng.choice(allowed))))                         # an empty mask
    m = np.zeros((H, W), bool)
    m[v0 - 1:, 1:max(3, v1 - 1)] = True
    preds.append((m, int(rng.choice(allowed))))                                              # mostly on void
    preds.append((_jitter(rng, img == group_label, 2), group_label))                         # mostly on a group region
    preds.append((_shape_mask(rng, H, W, 4, 6, 6, 9), int(rng.choice(allowed))))             # below 100 pixels
    preds.append((_shape_mask(rng, H, W, hmin, hmax, wmin, wmax), int(rng.choice([29, 7, 30]))))  # a label that is not evaluated
    if absent is not None:
      preds.append((_shape_mask(rng, H, W, hmin, hmax, wmin, wmax), absent))
    m = np.zeros((H, W), bool)
    m[r:r + 10, c:c + 20] = True
    preds.append((m, id100 // 1000))                         # 200 pixels around the 100: IoU exactly 0.5, which is no match
    preds.append((img == id99, id99 // 1000))                # the 99 pixels exactly: too small to count, so ignored
    if inst:
      twice = inst[rng.randint(len(inst))]
      preds.append((_jitter(rng, img == twice, 1), twice // 1000))                           # two predictions on one instance:
      preds.append((_jitter(rng, img == twice, 1), twice // 1000))                           # this one and the next
    if len(inst) >= 2:
      a, c = rng.choice(len(inst), 2, replace=False)
      preds.append(((img == inst[a]) | (img == inst[c]), inst[a] // 1000))                   # one prediction over two instances
    for i in inst:
      if rng.rand() < 0.8:
        preds.append((_jitter(rng, img == i, 1 + rng.randint(0, 3)), i // 1000))             # jittered copies
    while len(preds) < T and T > 20:                                                         # the 40-prediction scene: fill up
      preds.append((_shape_mask(rng, H, W, hmin, hmax, wmin, wmax), int(rng.choice(allowed))))
    for t, (m, label) in enumerate(preds[:T]):
      y[b, t], lab[b, t] = m, label
  # confidences: pairwise distinct multiples of 1e-4 in [0.05, 0.95), moved in the 7th decimal so that '%f' rounds them
  grid = (500 + rng.permutation(9000)[:B * T].reshape(B, T)) / 10000.0
  conf[:] = np.where(lab >= 0, grid + rng.randint(0, 4, (B, T)) * 2e-7, 0.0)
  names = ['city%d_%06d_000019.png' % (seed, b) for b in range(B)]
  return {'gt_ids': gt, 'y': y, 'label_id': lab, 'conf': conf, 'names': names}


def instance_scene(name, seed=None):
  kind, default_seed, B, H, W, T, n_inst = INSTANCE_SCENES[name]
  seed = default_seed if seed is None else int(seed)
  sc = ao.scene(seed) if kind == 'legacy' else _random_instance_scene(seed, B, H, W, T, n_inst)
  assert sc['gt_ids'].shape == (B, H, W) and sc['y'].shape == (B, T, H, W)
  return sc


def confidences_distinct(sc):
  """Within every evaluated class the written confidences of the scene's kept predictions (a label that is evaluated, a mask
  with pixels) are pairwise distinct after the '%f' rounding of the text file."""
  for label in EVALUATED:
    seen = [float('%f' % sc['conf'][b, t]) for b in range(sc['y'].shape[0]) for t in range(sc['y'].shape[1])
            if sc['label_id'][b, t] == label and sc['y'][b, t].any()]
    if len(seen) != len(set(seen)):
      return False
  return True


# ---- pixel level
def pixel_scene(name, seed=None):
  default_seed, B, H, W = PIXEL_SCENES[name]
  rng = np.random.RandomState(default_seed if seed is None else int(seed))
  pred, labels, ids = (np.stack(a) for a in zip(*[po.random_scene(rng, H, W, all_labels=True) for _ in range(B)]))
  if name.startswith('special'):
    pred[1] = 0
    r, c = H // 2, W // 2
    labels[2, r - 1:r + 2, c - 1:c + 2], ids[2, r - 1:r + 2, c - 1:c + 2] = 7, 7
    labels[2, r, c], ids[2, r, c] = 26, 26007            # an instance of exactly one pixel, predicted right
    pred[2, r - 1:r + 2, c - 1:c + 2] = 26
    assert (ids[2] == 26007).sum() == 1
  if name.startswith('zero'):
    pred[:] = 0
  assert (po.labels_of_ids(ids) == labels).all()
  return pred, labels, ids


# ---- orientation
def edge_masks():
  """uint8 [1,21,33]: the pixels where the reference's + 1e-8 / + 1e-7 terms and its strict > 0 tests decide the class."""
  img = np.zeros((1, 21, 33), np.uint8)
  img[0, 2, 29] = 1              # one pixel: it is its own centroid
  img[0, 5, 3:16] = 2            # 13 pixels wide, one high: the centroid is the pixel (5, 9)
  img[0, 8:19, 25] = 3           # 11 pixels high, one wide: the centroid is the pixel (13, 25)
  img[0, 10:17, 6:13] = 4        # 7 x 7: the centroid is the pixel (13, 9)
  img[0, 0, 0] = 5               # the centroid is (0, 0) exactly: both offsets are 0 and the + 1e-8 is all there is
  return img


def orientation_scene(name, seed=None):
  default_seed, B, H, W = ORIENTATION_SCENES[name]
  if default_seed is None:
    return edge_masks()
  rng = np.random.RandomState(default_seed if seed is None else int(seed))
  return lo.ellipse_ids(rng, B, H, W, 6).astype(np.uint8)


def orientation_margin(img):
  """Per pixel of one id image [H,W]: the distance of labels_oracle's pre-floor orientation value from an integer at the
  instance that covers the pixel (inf on the background), and the oracle's class image."""
  masks, _ = lo.separate_labels(img)
  cls, pre = lo.get_orientation(np.stack(masks))
  margin = np.full(img.shape, np.inf)
  for m, p in zip(masks, pre):
    on = m > 0
    margin[on] = np.abs(p[on] - np.round(p[on]))
  return margin, cls


# ---- the fixture files
def pack_masks(y):
  return np.packbits(np.asarray(y) != 0)


def unpack_masks(packed, shape, dtype=np.float32):
  n = int(np.prod(shape))
  return np.unpackbits(packed)[:n].reshape(shape).astype(dtype)


def instance_arrays(scenes):
  """{scene name: scene} -> the arrays of toolkit_instance.npz."""
  out = {'scenes': np.array(sorted(scenes))}
  for name, sc in scenes.items():
    assert sc['gt_ids'].min() >= 0 and sc['gt_ids'].max() < 65536
    out[name + '/gt_ids'] = sc['gt_ids'].astype(np.uint16)
    out[name + '/y_packed'] = pack_masks(sc['y'])
    out[name + '/y_shape'] = np.array(sc['y'].shape, np.int64)
    out[name + '/label_id'] = sc['label_id'].astype(np.int32)
    out[name + '/conf'] = sc['conf'].astype(np.float32)
    out[name + '/names'] = np.array(sc['names'])
  return out


def load_instance_scenes(npz):
  out = {}
  for name in [str(n) for n in npz['scenes']]:
    out[name] = {'gt_ids': npz[name + '/gt_ids'].astype(np.int32),
                 'y': unpack_masks(npz[name + '/y_packed'], tuple(npz[name + '/y_shape'])),
                 'label_id': npz[name + '/label_id'], 'conf': npz[name + '/conf'],
                 'names': [str(n) for n in npz[name + '/names']]}
  return out


def pixel_arrays(scenes):
  out = {'scenes': np.array(sorted(scenes))}
  for name, (pred, labels, ids) in scenes.items():
    out[name + '/pred'], out[name + '/gt_labels'], out[name + '/gt_ids'] = pred.astype(np.uint8), labels.astype(np.uint8), ids.astype(np.uint16)
    out[name + '/names'] = np.array(['pix%s_%06d_000019' % (name.replace('_', ''), b) for b in range(pred.shape[0])])
  return out


def load_pixel_scenes(npz):
  return {name: (npz[name + '/pred'], npz[name + '/gt_labels'], npz[name + '/gt_ids'].astype(np.int32), [str(n) for n in npz[name + '/names']])
          for name in [str(n) for n in npz['scenes']]}


def manifest_of(npz):
  return json.loads(str(npz['manifest']))


# ---- comparisons with a recorded result file, shared by the tests with and without a device
def _close(a, b, tol, what):
  a, b = float(a), float(b)
  if np.isnan(a) or np.isnan(b):
    assert np.isnan(a) and np.isnan(b), (what, a, b)
    return 0.0
  assert abs(a - b) <= tol, (what, a, b)
  return abs(a - b)


def assert_ap_result(got, recorded, tol, what=''):
  """got: the product's (or the oracle's) result dict, recorded: the toolkit's resultInstanceLevelSemanticLabeling.json.  Every
  key of the toolkit's file: the AP matrix and the averages within tol with NaN in the same places, the settings equal.
  Returns the largest difference seen."""
  ap, ref = np.array(got['resultApMatrix'], np.float64), np.array(recorded['resultApMatrix'], np.float64)
  assert ap.shape == ref.shape == (1, 8, 10), (what, ap.shape, ref.shape)
  assert np.array_equal(np.isnan(ap), np.isnan(ref)), (what, 'NaN pattern')
  worst = float(np.nanmax(np.abs(ap - ref))) if np.isfinite(ref).any() else 0.0
  assert worst <= tol, (what, worst)
  assert sorted(recorded['averages']) == ['allAp', 'allAp50%', 'classes'] and sorted(got['averages']) == sorted(recorded['averages'])
  for k in ('allAp', 'allAp50%'):
    worst = max(worst, _close(got['averages'][k], recorded['averages'][k], tol, (what, k)))
  assert sorted(got['averages']['classes']) == sorted(recorded['averages']['classes'])
  for name, rec in recorded['averages']['classes'].items():
    assert sorted(rec) == ['ap', 'ap50%']
    for k in rec:
      worst = max(worst, _close(got['averages']['classes'][name][k], rec[k], tol, (what, name, k)))
  for k in ('overlaps', 'minRegionSizes', 'distanceThresholds', 'minStereoDensities', 'instLabels'):
    if k in got:
      assert got[k] == recorded[k], (what, k)
  return worst


def assert_pixel_result(got, recorded, what='', rel=1e-12):
  """got: the product's result dict, recorded: the toolkit's resultSemanticLabeling.json.  The matrix and the label table
  equal, the scores under pixel_oracle.same_scores, the priors within the same relative bound.  Returns the largest relative
  difference seen."""
  assert got['confMatrix'] == recorded['confMatrix'], (what, 'confMatrix')
  assert got['labels'] == recorded['labels'], (what, 'labels')
  po.same_scores(got, recorded, rel=rel)
  assert sorted(got['priors']) == sorted(recorded['priors'])
  for name, p in recorded['priors'].items():
    po._same(got['priors'][name], p, rel, (what, 'priors', name))
  pairs = [(got[k][n], recorded[k][n]) for k in po.SCORE_KEYS + ['priors'] for n in recorded[k]] + [(got[k], recorded[k]) for k in po.AVERAGE_KEYS]
  return max([abs(a - b) / max(abs(a), abs(b)) for a, b in pairs if a == a and a != b] + [0.0])  # the largest relative difference
