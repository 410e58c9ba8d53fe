"""Float64 NumPy oracle of the Cityscapes instance-level evaluation (the reference's
data_api/cityscapes_scripts/evaluation/evalInstanceLevelSemanticLabeling.py, cited as :line; instances2dict.py, instance.py):
the ground-truth instances of an image, the assignment of predictions to them (:260-353), the matching per class and overlap
threshold (:356-551) and the averages (:553-579), restated loop by loop on pixel arrays — one count_nonzero per prediction
and ground-truth instance, one np.append per example — and slow on purpose.  It shares no code with analysis.py.  The script
itself runs once translated to Python 3: oracle/toolkit_fixtures.py recorded its result files on seven scenes as
tests/golden/toolkit_instance.{npz,json}, and tests/test_toolkit_fixtures.py holds run() to them (observed difference: 0).  `COUNTERS`
records which branches a run took, so that a test can assert that its scene reached them.  Also here: a seeded scene generator
and a 16-bit PNG writer for the ground truth of the file-route tests."""
import collections
import os
import struct
import zlib

import numpy as np

# (name, id) of the labels with instances that are evaluated, in the order of helpers/labels.py
INST_LABELS = [('person', 24), ('rider', 25), ('car', 26), ('truck', 27), ('bus', 28), ('train', 31), ('motorcycle', 32),
               ('bicycle', 33)]
# ids of the labels with ignoreInEval in helpers/labels.py (-1, license plate, cannot be stored in the image)
VOID_IDS = [0, 1, 2, 3, 4, 5, 6, 9, 10, 14, 15, 16, 18, 29, 30, -1]
OVERLAPS = np.arange(0.5, 1., 0.05)   # :134
MIN_REGION = 100                      # :136, first entry (no distances: :386-389)

COUNTERS = collections.Counter()
# the branches a set of scenes has to take before its AP says anything about the evaluation (keys of COUNTERS)
BRANCHES = ('pred_on_void', 'void_ignored',                      # void pixels under a prediction, enough of them to ignore it
            'matched_a_group', 'group_pixels_ignored',
            'matched_a_small_instance', 'small_instance_pixels_ignored',
            'hard_false_negative', 'duplicate_match', 'false_positive', 'class_with_gt_only', 'class_with_neither',
            'pred_label_not_evaluated', 'pred_empty', 'equal_score_true_and_false')


def gt_instances(gt):
  """instances2dict.py:37-40 + instance.py: {label id: [instance dict]} for every distinct value of the image."""
  out = {}
  for value in np.unique(gt):
    value = int(value)
    label = value if value < 1000 else int(value / 1000)
    out.setdefault(label, []).append({'id': value, 'label': label, 'pixels': int((gt == value).sum())})
  return out


def assign(gt, preds):
  """:260-353.  gt: int [H,W]; preds: list of (mask [H,W], label id, confidence).  -> (gt instances per evaluated label
  name, each with its list of touching predictions; kept predictions per label name, each with its touching instances)."""
  names = {i: n for n, i in INST_LABELS}
  orig = gt_instances(gt)
  gts = {n: [dict(g, matched=[]) for g in orig.get(i, [])] for n, i in INST_LABELS}
  out_preds = {n: [] for n, _ in INST_LABELS}
  void = np.isin(gt, VOID_IDS)
  for mask, label, conf in preds:
    if int(label) not in names:
      COUNTERS['pred_label_not_evaluated'] += 1
      continue
    name = names[int(label)]
    inst = mask != 0
    n_pix = int(np.count_nonzero(inst))
    if not n_pix:
      COUNTERS['pred_empty'] += 1
      continue
    p = {'label': int(label), 'pixels': n_pix, 'conf': conf, 'void': int(np.count_nonzero(np.logical_and(void, inst)))}
    if p['void']:
      COUNTERS['pred_on_void'] += 1
    touching = []
    for gi, g in enumerate(gts[name]):
      inter = int(np.count_nonzero(np.logical_and(gt == g['id'], inst)))
      if inter > 0:
        touching.append({'id': g['id'], 'pixels': g['pixels'], 'inter': inter})
        g['matched'].append(dict(p, inter=inter))
    p['touching'] = touching
    out_preds[name].append(p)
  return gts, out_preds


def evaluate(matches):
  """:356-551 for a list of assign() results -> ap [1, 8, 10]."""
  ap = np.zeros((1, len(INST_LABELS), len(OVERLAPS)))
  for oi, th in enumerate(OVERLAPS):
    for li, (name, _) in enumerate(INST_LABELS):
      y_true, y_score = np.empty(0), np.empty(0)
      hard_fns = 0
      have_gt = have_pred = False
      for gts_all, preds_all in matches:
        preds = preds_all[name]
        gts = [g for g in gts_all[name] if g['id'] >= 1000 and g['pixels'] >= MIN_REGION]
        have_gt = have_gt or bool(gts)
        have_pred = have_pred or bool(preds)
        cur_true = np.ones(len(gts))
        cur_score = np.ones(len(gts)) * (-float('inf'))
        cur_match = np.zeros(len(gts), dtype=bool)
        for gi, g in enumerate(gts):
          found = False
          for p in g['matched']:
            overlap = float(p['inter']) / (g['pixels'] + p['pixels'] - p['inter'])
            if overlap > th:
              if cur_match[gi]:  # a second prediction on this instance: the lower score is a false positive
                COUNTERS['duplicate_match'] += 1
                hi, lo = max(cur_score[gi], p['conf']), min(cur_score[gi], p['conf'])
                cur_score[gi] = hi
                cur_true = np.append(cur_true, 0)
                cur_score = np.append(cur_score, lo)
                cur_match = np.append(cur_match, True)
              else:
                found = True
                cur_match[gi] = True
                cur_score[gi] = p['conf']
          if not found:
            COUNTERS['hard_false_negative'] += 1
            hard_fns += 1
        cur_true = cur_true[cur_match]
        cur_score = cur_score[cur_match]
        for p in preds:
          found = False
          for g in p['touching']:
            overlap = float(g['inter']) / (g['pixels'] + p['pixels'] - g['inter'])
            if overlap > th:
              found = True
              if g['id'] < 1000:
                COUNTERS['matched_a_group'] += 1
              elif g['pixels'] < MIN_REGION:
                COUNTERS['matched_a_small_instance'] += 1
              break
          if not found:
            n_ignore = p['void']
            for g in p['touching']:
              if g['id'] < 1000:
                COUNTERS['group_pixels_ignored'] += 1
                n_ignore += g['inter']
              if g['pixels'] < MIN_REGION:
                COUNTERS['small_instance_pixels_ignored'] += 1
                n_ignore += g['inter']
            if float(n_ignore) / p['pixels'] <= th:
              COUNTERS['false_positive'] += 1
              cur_true = np.append(cur_true, 0)
              cur_score = np.append(cur_score, p['conf'])
            else:
              COUNTERS['void_ignored' if p['void'] else 'other_ignored'] += 1
        y_true = np.append(y_true, cur_true)
        y_score = np.append(y_score, cur_score)
      if have_gt and have_pred:
        order = np.argsort(y_score)
        s_sorted, t_sorted = y_score[order], y_true[order]
        t_cum = np.cumsum(t_sorted)
        _, first = np.unique(s_sorted, return_index=True)
        n_pr = len(first) + 1
        n_ex, n_true = len(s_sorted), t_cum[-1]
        precision, recall = np.zeros(n_pr), np.zeros(n_pr)
        t_cum = np.append(t_cum, 0)  # index -1 reads this zero
        for ri, si in enumerate(first):
          below = t_cum[si - 1]
          tp = n_true - below
          fp = n_ex - si - tp
          fn = below + hard_fns
          precision[ri] = float(tp) / (tp + fp)
          recall[ri] = float(tp) / (tp + fn)
          end = first[ri + 1] if ri + 1 < len(first) else n_ex
          if 0 < t_sorted[si:end].sum() < end - si:
            COUNTERS['equal_score_true_and_false'] += 1
        precision[-1], recall[-1] = 1., 0.
        r = np.append(np.append(recall[0], recall), 0.)
        ap[0, li, oi] = np.dot(precision, np.convolve(r, [-0.5, 0, 0.5], 'valid'))
      elif have_gt:
        COUNTERS['class_with_gt_only'] += 1
        ap[0, li, oi] = 0.0
      else:
        COUNTERS['class_with_neither'] += 1
        ap[0, li, oi] = float('nan')
  return ap


def averages(ap):
  """:553-579 without distances."""
  o50 = np.where(np.isclose(OVERLAPS, 0.5))
  avg = {'allAp': np.nanmean(ap[0, :, :]), 'allAp50%': np.nanmean(ap[0, :, o50]), 'classes': {}}
  for li, (name, _) in enumerate(INST_LABELS):
    avg['classes'][name] = {'ap': np.average(ap[0, li, :]), 'ap50%': np.average(ap[0, li, o50])}
  return avg


def run(gt_images, preds_per_image):
  """(ap, averages) of a list of ground-truth images and, per image, a list of (mask, label id, confidence)."""
  ap = evaluate([assign(g, p) for g, p in zip(gt_images, preds_per_image)])
  return ap, averages(ap)


def read_result_files(text_file, read_mask):
  """:165-189: the (mask, label id, confidence) list of one prediction text file; read_mask(path) -> array."""
  preds = []
  for line in open(text_file):
    parts = line.split(' ')
    assert len(parts) == 3 and not os.path.isabs(parts[0])
    preds.append((read_mask(os.path.join(os.path.dirname(text_file), parts[0])), int(float(parts[1])), float(parts[2])))
  return preds


def encode_gray16(img, filter_type=0):
  """uint16 [H,W] -> a 16-bit greyscale PNG with the given filter type on every row (0 .. 4), filtered as the PNG
  specification (section 9) says, byte by byte."""
  img = np.ascontiguousarray(img, dtype='>u2')
  H, W = img.shape
  rows = np.frombuffer(img.tobytes(), np.uint8).reshape(H, 2 * W).astype(int)
  raw = bytearray()
  for r in range(H):
    raw.append(filter_type)
    for i in range(2 * W):
      a = rows[r, i - 2] if i >= 2 else 0
      b = rows[r - 1, i] if r > 0 else 0
      c = rows[r - 1, i - 2] if (r > 0 and i >= 2) else 0
      if filter_type == 0:
        pred = 0
      elif filter_type == 1:
        pred = a
      elif filter_type == 2:
        pred = b
      elif filter_type == 3:
        pred = (a + b) // 2
      else:
        p = a + b - c
        pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
        pred = a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)
      raw.append((rows[r, i] - pred) % 256)
  chunk = lambda tag, data: struct.pack('>I', len(data)) + tag + data + struct.pack('>I', zlib.crc32(tag + data) & 0xffffffff)
  return (b'\x89PNG\r\n\x1a\n' + chunk(b'IHDR', struct.pack('>IIBBBBB', W, H, 16, 0, 0, 0, 0)) +
          chunk(b'IDAT', zlib.compress(bytes(raw))) + chunk(b'IEND', b''))


# ---- the scene: 3 images of 96 x 160, 8 predictions each
SCENE_H, SCENE_W, SCENE_T = 96, 160, 8
SCENE_NAMES = ['aachen_000001_000019.png', 'aachen_000002_000019.png', 'bochum_000001_000019']


def _rect(a, box, value):
  r0, r1, c0, c1 = box
  a[r0:r1, c0:c1] = value


def scene(seed=0):
  """-> dict: gt_ids int32 [3,96,160], y float32 [3,8,96,160] (binary), label_id int32 [3,8], conf float32 [3,8].  The seed
  only jitters the scores in their 5th decimal (so that '%f' rounds them) and the background ids; the geometry is fixed, and
  with it the branches the evaluation takes (tests/test_cityscapes_ap.py asserts them from COUNTERS):
    image 0  cars 26001 (two predictions above IoU 0.5 -> the lower one a false positive; one of them ties in score with a
             false positive on the road) and 26002 (no prediction: a hard false negative), a car GROUP (raw 26) under a
             prediction, an 80-pixel person 24001 under a prediction (ignored, not a false positive), a person 24002 nobody
             predicts, a truck 27001 (truck: ground truth and no prediction anywhere -> AP 0), a void band (raw 3) under a
             prediction, a caravan 29001 (not void: 29001 is not a label id), a prediction with label -1 and an empty mask;
    image 1  a rider and a car found, a person prediction on the pavement;
    image 2  one car found at IoU 0.6, void raw 0 around the border.
  bus, train, motorcycle, bicycle: neither ground truth nor prediction -> NaN."""
  rng = np.random.RandomState(seed)
  H, W, T = SCENE_H, SCENE_W, SCENE_T
  gt = np.zeros((3, H, W), np.int32)
  y = np.zeros((3, T, H, W), np.float32)
  lab = np.full((3, T), -1, np.int32)
  conf = np.zeros((3, T), np.float32)

  def pred(b, t, box, label, score):
    if box is not None:
      _rect(y[b, t], box, 1.0)
    lab[b, t] = label
    conf[b, t] = score

  gt[0] = 7 + rng.randint(0, 2)                  # road / sidewalk
  _rect(gt[0], (10, 40, 10, 60), 26001)          # 1500 px
  _rect(gt[0], (50, 80, 20, 70), 26002)          # 1500 px, never predicted
  _rect(gt[0], (10, 40, 100, 150), 26)           # a car group
  _rect(gt[0], (60, 68, 100, 110), 24001)        # 80 px: below the minimum region size
  _rect(gt[0], (45, 85, 120, 140), 24002)
  _rect(gt[0], (45, 60, 75, 95), 27001)
  _rect(gt[0], (2, 8, 70, 90), 29001)            # caravan instance
  _rect(gt[0], (88, 96, 0, 160), 3)              # void
  pred(0, 0, (10, 40, 12, 60), 26, 0.9)          # IoU 1440 / 1500 with 26001
  pred(0, 1, (10, 38, 10, 58), 26, 0.6)          # IoU 1344 / 1500 with 26001 as well
  pred(0, 2, (12, 38, 102, 148), 26, 0.8)        # inside the group: 1196 / 1500
  pred(0, 3, (59, 69, 99, 111), 24, 0.7)         # 120 px, 80 of them on the small person
  pred(0, 4, (84, 96, 20, 60), 26, 0.5)          # 480 px, 320 of them void
  pred(0, 5, (20, 30, 70, 80), -1, 0.95)         # not written
  pred(0, 6, None, 26, 0.9)                      # empty
  pred(0, 7, (70, 86, 75, 98), 26, 0.9)          # on the road: false, same score as prediction 0
  gt[1] = 8 + 3 * rng.randint(0, 2)              # sidewalk / building
  _rect(gt[1], (20, 60, 30, 60), 25001)
  _rect(gt[1], (10, 50, 90, 150), 26001)
  pred(1, 0, (22, 60, 30, 58), 25, 0.75)
  pred(1, 1, (10, 50, 90, 150), 26, 0.95)
  pred(1, 2, (70, 90, 40, 70), 24, 0.65)
  pred(1, 3, (0, 4, 0, 4), 29, 0.9)              # a label that is not evaluated
  gt[2] = 0
  _rect(gt[2], (4, 92, 4, 156), 11)
  _rect(gt[2], (64, 90, 5, 45), 26005)
  pred(2, 0, (64, 90, 17, 50), 26, 0.55)         # inter 26 x 28 = 728, union 1040 + 858 - 728 = 1170: IoU 0.62
  conf = (conf + np.where(conf > 0, rng.randint(0, 4, conf.shape) * 2e-7, 0)).astype(np.float32)
  conf[0, 7] = conf[0, 0]
  return {'gt_ids': gt, 'y': y, 'label_id': lab, 'conf': conf, 'names': list(SCENE_NAMES)}


def scene_preds(sc):
  """The scene as the oracle's input: per image the (mask, label id, float('%f' % conf)) list of the written predictions."""
  out = []
  for b in range(sc['y'].shape[0]):
    out.append([(sc['y'][b, t], int(sc['label_id'][b, t]), float('%f' % sc['conf'][b, t])) for t in range(sc['y'].shape[1])])
  return out
