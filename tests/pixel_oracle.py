"""NumPy restatement of the Cityscapes pixel-level evaluation (data_api/cityscapes_scripts/evaluation/
evalPixelLevelSemanticLabeling.py: evaluatePair :532-615, the score functions :216-338, getScoreAverage :273-282,
generateInstanceStats :171-202), written from those lines with plain loops over np.unique and a [34,34] matrix; the test
helper of test_pixel_eval*.py.  The label table (helpers/labels.py) and avgClassSize (:135-146) are data.  The script itself
runs once translated to Python 3 (its pure-Python pair loop): oracle/toolkit_fixtures.py recorded its result files on four
scenes as tests/golden/toolkit_pixel.{npz,json}, and tests/test_toolkit_fixtures.py holds evaluate() to them — matrix equal,
scores within same_scores (observed difference: 0)."""
import math
import struct
import zlib

import numpy as np

NUM_LABELS = 34
# id: (name, category, hasInstances, ignoreInEval)
LABELS = {
    0: ('unlabeled', 'void', 0, 1), 1: ('ego vehicle', 'void', 0, 1), 2: ('rectification border', 'void', 0, 1),
    3: ('out of roi', 'void', 0, 1), 4: ('static', 'void', 0, 1), 5: ('dynamic', 'void', 0, 1), 6: ('ground', 'void', 0, 1),
    7: ('road', 'flat', 0, 0), 8: ('sidewalk', 'flat', 0, 0), 9: ('parking', 'flat', 0, 1), 10: ('rail track', 'flat', 0, 1),
    11: ('building', 'construction', 0, 0), 12: ('wall', 'construction', 0, 0), 13: ('fence', 'construction', 0, 0),
    14: ('guard rail', 'construction', 0, 1), 15: ('bridge', 'construction', 0, 1), 16: ('tunnel', 'construction', 0, 1),
    17: ('pole', 'object', 0, 0), 18: ('polegroup', 'object', 0, 1), 19: ('traffic light', 'object', 0, 0),
    20: ('traffic sign', 'object', 0, 0), 21: ('vegetation', 'nature', 0, 0), 22: ('terrain', 'nature', 0, 0),
    23: ('sky', 'sky', 0, 0), 24: ('person', 'human', 1, 0), 25: ('rider', 'human', 1, 0), 26: ('car', 'vehicle', 1, 0),
    27: ('truck', 'vehicle', 1, 0), 28: ('bus', 'vehicle', 1, 0), 29: ('caravan', 'vehicle', 1, 1),
    30: ('trailer', 'vehicle', 1, 1), 31: ('train', 'vehicle', 1, 0), 32: ('motorcycle', 'vehicle', 1, 0),
    33: ('bicycle', 'vehicle', 1, 0)}
CATEGORIES = ['void', 'flat', 'construction', 'object', 'nature', 'sky', 'human', 'vehicle']
AVG_CLASS_SIZE = {'bicycle': 4672.3249222261, 'caravan': 36771.8241758242, 'motorcycle': 6298.7200839748,
                  'rider': 3930.4788056518, 'bus': 35732.1511111111, 'train': 67583.7075812274, 'car': 12794.0202738185,
                  'person': 3462.4756337644, 'truck': 27855.1264367816, 'trailer': 16926.9763313609}
THING_LABELS = [24, 25, 26, 27, 28, 31, 32, 33]  # channel c >= 1 of the pre-stage's semantic map -> THING_LABELS[c - 1]
SCORE_KEYS = ['classScores', 'classInstScores', 'categoryScores', 'categoryInstScores']
AVERAGE_KEYS = ['averageScoreClasses', 'averageScoreInstClasses', 'averageScoreCategories', 'averageScoreInstCategories']


def new_instance_stats():
  """:171-202"""
  st = {'classes': {}, 'categories': {}}
  for lid in range(NUM_LABELS):
    name, _, has, ign = LABELS[lid]
    if has and not ign:
      st['classes'][name] = {'tp': 0.0, 'tpWeighted': 0.0, 'fn': 0.0, 'fnWeighted': 0.0}
  for cat in CATEGORIES:
    ids, every = [], True
    for lid in range(NUM_LABELS):
      if LABELS[lid][1] != cat:
        continue
      if not LABELS[lid][2]:
        every = False
        break
      ids.append(lid)
    if every:
      st['categories'][cat] = {'tp': 0.0, 'tpWeighted': 0.0, 'fn': 0.0, 'fnWeighted': 0.0, 'labelIds': ids}
  return st


def new_state():
  return {'conf': np.zeros((NUM_LABELS, NUM_LABELS), np.int64), 'inst': new_instance_stats(), 'pixels': 0}


def labels_of_ids(ids):
  """How *_instanceIds.png encodes the label: the value itself below 1000, else value // 1000."""
  ids = np.asarray(ids).astype(np.int64)
  return np.where(ids < 1000, ids, ids // 1000)


def evaluate_pair(pred, gt_labels, gt_ids, state):
  """:532-615 for one image (pred, gt_labels, gt_ids [H,W]); grows state in place."""
  pred, gt_labels, gt_ids = (np.asarray(a).astype(np.int64) for a in (pred, gt_labels, gt_ids))
  assert pred.shape == gt_labels.shape == gt_ids.shape
  for g in np.unique(gt_labels):
    assert 0 <= g < NUM_LABELS, 'Unknown label with id %d' % g  # :570-571
    for p in np.unique(pred[gt_labels == g]):
      state['conf'][g, p] += int(((gt_labels == g) & (pred == p)).sum())  # :573
  state['pixels'] += pred.size
  st = state['inst']
  cat_masks = {c: np.isin(pred, st['categories'][c]['labelIds']) for c in st['categories']}  # :577-579
  for inst_id in np.unique(gt_ids[gt_ids > 1000]):  # :581
    label = int(inst_id) // 1000
    name, cat, _, ign = LABELS[label]
    if ign:
      continue
    mask = gt_ids == inst_id
    size = int(mask.sum())
    tp = int((pred[mask] == label).sum())
    weight = AVG_CLASS_SIZE[name] / float(size)
    rec = st['classes'][name]
    rec['tp'] += tp
    rec['fn'] += size - tp
    rec['tpWeighted'] += float(tp) * weight
    rec['fnWeighted'] += float(size - tp) * weight
    if cat in st['categories']:
      ctp = int((mask & cat_masks[cat]).sum())
      rec = st['categories'][cat]
      rec['tp'] += ctp
      rec['fn'] += size - ctp
      rec['tpWeighted'] += float(ctp) * weight
      rec['fnWeighted'] += float(size - ctp) * weight
  return state


def instance_counts(pred, gt_ids):
  """What the confusion kernel reports per catalogue slot, for EVERY distinct id of one image in ascending order:
  [(id, pixels, tp, cat_tp)] with tp = pixels of the id predicted as id // 1000 and cat_tp = those predicted inside the
  instance category (human {24, 25}, vehicle {26 .. 33}) of id // 1000, 0 where that label is in neither."""
  pred, gt_ids = np.asarray(pred).astype(np.int64), np.asarray(gt_ids).astype(np.int64)
  cats = {c: r['labelIds'] for c, r in new_instance_stats()['categories'].items()}
  out = []
  for inst_id in np.unique(gt_ids):
    mask = gt_ids == inst_id
    label = int(inst_id) // 1000
    members = [ids for ids in cats.values() if label in ids]
    ctp = int(np.isin(pred[mask], members[0]).sum()) if members else 0
    out.append((int(inst_id), int(mask.sum()), int((pred[mask] == label).sum()), ctp))
  return out


def _ratio(tp, fp, fn):
  denom = tp + fp + fn
  return float('nan') if denom == 0 else float(tp) / denom


def scores(conf, inst):
  """:216-338 and the averages (:273-282, :353-356)."""
  conf = np.asarray(conf).astype(np.int64)
  valid = [l for l in range(NUM_LABELS) if not LABELS[l][3]]
  out = {k: {} for k in SCORE_KEYS}
  for l in range(NUM_LABELS):
    name = LABELS[l][0]
    if LABELS[l][3]:
      out['classScores'][name] = out['classInstScores'][name] = float('nan')
      continue
    tp = int(conf[l, l])
    fn = sum(int(conf[l, p]) for p in range(NUM_LABELS)) - tp
    fp = sum(int(conf[g, l]) for g in valid if g != l)
    out['classScores'][name] = _ratio(tp, fp, fn)
    out['classInstScores'][name] = (_ratio(inst['classes'][name]['tpWeighted'], fp, inst['classes'][name]['fnWeighted'])
                                    if name in inst['classes'] else float('nan'))
  for cat in CATEGORIES:
    members = [l for l in valid if LABELS[l][1] == cat]
    outside = [l for l in valid if LABELS[l][1] != cat]
    if members:
      tp = sum(int(conf[g, p]) for g in members for p in members)
      fn = sum(int(conf[g, p]) for g in members for p in range(NUM_LABELS)) - tp
      fp = sum(int(conf[g, p]) for g in outside for p in members)
      out['categoryScores'][cat] = _ratio(tp, fp, fn)
    else:
      out['categoryScores'][cat] = float('nan')
    if cat in inst['categories']:
      fp = sum(int(conf[g, p]) for g in outside for p in inst['categories'][cat]['labelIds'])
      out['categoryInstScores'][cat] = _ratio(inst['categories'][cat]['tpWeighted'], fp, inst['categories'][cat]['fnWeighted'])
    else:
      out['categoryInstScores'][cat] = float('nan')
  for key, src in zip(AVERAGE_KEYS, SCORE_KEYS):
    out[key] = average(out[src])
  return out


def average(score_dict):
  """:273-282"""
  vals = [v for v in score_dict.values() if not math.isnan(v)]
  return float('nan') if not vals else sum(vals, 0.0) / len(vals)


def evaluate(preds, gt_labels, gt_ids):
  """Whole lists of images -> (state, scores)."""
  state = new_state()
  for p, l, i in zip(preds, gt_labels, gt_ids):
    evaluate_pair(p, l, i, state)
  assert int(state['conf'].sum()) == state['pixels']  # :462-463
  return state, scores(state['conf'], state['inst'])


def argmax_labels(sem_h):
  """sem_h [..., C] at full size -> label ids: the first maximum, channel 0 -> 0, channel c -> THING_LABELS[c - 1]."""
  return np.array([0] + THING_LABELS, np.int64)[np.argmax(sem_h, axis=-1)]


def top2_gap(sem_h):
  s = np.sort(sem_h, axis=-1)
  return s[..., -1] - s[..., -2]


def same_scores(a, b, rel=1e-12):
  """The score dicts a, b agree: NaN in the same places, else within rel."""
  for key in SCORE_KEYS:
    assert sorted(a[key]) == sorted(b[key]), key
    for name in a[key]:
      _same(a[key][name], b[key][name], rel, (key, name))
  for key in AVERAGE_KEYS:
    _same(a[key], b[key], rel, key)


def _same(x, y, rel, what):
  if math.isnan(x) or math.isnan(y):
    assert math.isnan(x) and math.isnan(y), (what, x, y)
  else:
    assert abs(x - y) <= rel * max(abs(x), abs(y)), (what, x, y)


# ---- inputs the tests share ----
def random_scene(rng, H, W, n_inst=12, all_labels=True, wrong=0.3):
  """A ground truth of horizontal label bands with rectangular instances on top and a prediction that copies it except for
  rectangles of other labels: (pred uint8, gt_labels uint8, gt_ids int32) [H,W].  all_labels: every label 0 .. 33 occurs in
  both (the first 34 pixels of a shuffled position list are forced)."""
  labels = rng.randint(0, 24, (H, 1)).repeat(W, axis=1)
  ids = labels.copy()
  serial = {}
  for _ in range(n_inst):
    lab = int(rng.choice([24, 25, 26, 27, 28, 29, 30, 31, 32, 33]))
    h, w = rng.randint(1, max(2, H // 3)), rng.randint(1, max(2, W // 3))
    r, c = rng.randint(0, H - h + 1), rng.randint(0, W - w + 1)
    k = serial.get(lab, 0)
    serial[lab] = k + 1
    labels[r:r + h, c:c + w] = lab
    ids[r:r + h, c:c + w] = lab * 1000 + k if rng.rand() > 0.15 else lab  # some regions are groups: the bare label
  pred = labels.copy()
  for _ in range(int(wrong * 20)):
    h, w = rng.randint(1, max(2, H // 4)), rng.randint(1, max(2, W // 2))
    r, c = rng.randint(0, H - h + 1), rng.randint(0, W - w + 1)
    pred[r:r + h, c:c + w] = rng.randint(0, NUM_LABELS)
  if all_labels:
    pos = rng.permutation(H * W)
    for l in range(NUM_LABELS):
      labels.flat[pos[l]] = l
      ids.flat[pos[l]] = l if l < 24 else l * 1000 + 500
      pred.flat[pos[NUM_LABELS + l]] = l
  return pred.astype(np.uint8), labels.astype(np.uint8), ids.astype(np.int32)


def encode_png(img, bits):
  """uint8 / uint16 [H,W] -> an 8- or 16-bit greyscale PNG, filter type 0 on every row."""
  img = np.ascontiguousarray(img, dtype='>u2' if bits == 16 else 'u1')
  H, W = img.shape
  raw = b''.join(b'\x00' + img[r].tobytes() for r in range(H))
  chunk = lambda tag, data: struct.pack('>I', len(data)) + tag + data + struct.pack('>I', zlib.crc32(tag + data) & 0xffffffff)
  return (b'\x89PNG\r\n\x1a\n' + chunk(b'IHDR', struct.pack('>IIBBBBB', W, H, bits, 0, 0, 0, 0)) +
          chunk(b'IDAT', zlib.compress(raw)) + chunk(b'IEND', b''))
