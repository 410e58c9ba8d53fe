"""The Cityscapes pixel-level evaluation without a device: the NumPy oracle (tests/pixel_oracle.py) pinned by a hand-computed
image and by properties of the toolkit's definitions, analysis.cityscapes_pixel_scores against the oracle (integers equal,
float64 scores within 1e-12 relative, NaN in the same places), the JSON keys, the command line's file pairing on tiny PNG
files, and every refusal of ops.sem_labels / ops.pixel_confusion — all of which happen before any launch."""
import json
import math
import os

import numpy as np
import pytest
import torch

import analysis
import cityscapes_pixel
import pixel_oracle as po
import ra_native as rn
import ra_ops as ops

W_PERSON = 3462.4756337644
W_CAR = 12794.0202738185


def _hand_image():
  gt = np.array([[7, 7, 7, 24, 24, 24],
                 [7, 7, 7, 24, 24, 24],
                 [7, 7, 26, 26, 26, 26],
                 [0, 0, 26, 26, 26, 26]])
  ids = np.where(gt == 24, 24001, np.where(gt == 26, 26000, gt))
  pred = np.array([[7, 7, 24, 24, 24, 7],
                   [7, 7, 7, 24, 25, 26],
                   [7, 26, 26, 26, 26, 24],
                   [7, 26, 26, 26, 0, 26]])
  return pred, gt, ids


def test_oracle_on_a_hand_computed_image():
  pred, gt, ids = _hand_image()
  state, sc = po.evaluate([pred], [gt], [ids])
  want = {(7, 7): 6, (7, 24): 1, (7, 26): 1, (24, 24): 3, (24, 7): 1, (24, 25): 1, (24, 26): 1, (26, 26): 6, (26, 24): 1,
          (26, 0): 1, (0, 7): 1, (0, 26): 1}
  conf = np.zeros((34, 34), np.int64)
  for (g, p), n in want.items():
    conf[g, p] = n
  assert (state['conf'] == conf).all() and state['conf'].sum() == 24
  # class IoU: tp / (tp + fp + fn); the two pixels whose ground truth is 'unlabeled' cost road and car nothing
  cs = sc['classScores']
  assert cs['road'] == 6 / 9.0 and cs['person'] == 3 / 8.0 and cs['rider'] == 0.0 and cs['car'] == 6 / 10.0
  for name in ('sidewalk', 'truck', 'sky', 'unlabeled', 'caravan'):
    assert math.isnan(cs[name])
  assert sc['averageScoreClasses'] == (6 / 9.0 + 3 / 8.0 + 0.0 + 6 / 10.0) / 4
  # iIoU: person 24001 has 6 pixels, 3 right; car 26000 has 8 pixels, 6 right; fp from the matrix
  wp, wc = W_PERSON / 6.0, W_CAR / 8.0
  ci = sc['classInstScores']
  assert ci['person'] == pytest.approx(3 * wp / (3 * wp + 2 + 3 * wp), rel=1e-15)
  assert ci['car'] == pytest.approx(6 * wc / (6 * wc + 2 + 2 * wc), rel=1e-15)
  assert ci['rider'] == 0.0 and math.isnan(ci['truck']) and math.isnan(ci['road'])
  assert state['inst']['classes']['person'] == {'tp': 3.0, 'fn': 3.0, 'tpWeighted': 3.0 * wp, 'fnWeighted': 3.0 * wp}
  # categories
  cat = sc['categoryScores']
  assert cat['flat'] == 6 / 9.0 and cat['human'] == 4 / 8.0 and cat['vehicle'] == 6 / 10.0
  for name in ('void', 'construction', 'object', 'nature', 'sky'):
    assert math.isnan(cat[name])
  cati = sc['categoryInstScores']
  assert cati['human'] == pytest.approx(4 * wp / (4 * wp + 2 + 2 * wp), rel=1e-15)
  assert cati['vehicle'] == pytest.approx(6 * wc / (6 * wc + 2 + 2 * wc), rel=1e-15)
  assert math.isnan(cati['flat']) and math.isnan(cati['void'])
  assert sc['averageScoreCategories'] == (6 / 9.0 + 0.5 + 0.6) / 3
  assert po.instance_counts(pred, ids) == [(0, 2, 0, 0), (7, 8, 0, 0), (24001, 6, 3, 4), (26000, 8, 6, 6)]


def test_oracle_properties():
  rng = np.random.RandomState(0)
  pred, gt, ids = po.random_scene(rng, 40, 60)
  # a perfect prediction: IoU 1 for the evaluated classes that occur, NaN for the others
  state, sc = po.evaluate([gt], [gt], [ids])
  assert state['conf'].sum() == gt.size == state['pixels']
  for l in range(34):
    name, _, _, ign = po.LABELS[l]
    assert math.isnan(sc['classScores'][name]) if ign else sc['classScores'][name] == 1.0
  only = np.full((8, 8), 7)
  _, sc = po.evaluate([only], [only], [only])
  assert sc['classScores']['road'] == 1.0 and math.isnan(sc['classScores']['sidewalk']) and sc['averageScoreClasses'] == 1.0
  # predicting an ignored label onto a valid one: a false negative there, a false positive nowhere
  p2 = only.copy()
  p2[0, :4] = 1
  _, sc = po.evaluate([p2], [only], [only])
  assert sc['classScores']['road'] == 60 / 64.0 and sc['averageScoreClasses'] == 60 / 64.0
  # pixels whose ground truth is ignored give no false positive
  g3 = only.copy()
  g3[:2] = 3
  _, sc = po.evaluate([only], [g3], [g3])
  assert sc['classScores']['road'] == 1.0
  # a caravan instance (label 29, ignored) is skipped, id 1000 is skipped, 24000 counts
  g4 = np.full((4, 8), 7)
  i4 = g4.copy()
  g4[0], i4[0] = 29, 29001
  g4[1], i4[1] = 1, 1000
  g4[2], i4[2] = 24, 24000
  state, sc = po.evaluate([g4], [g4], [i4])
  assert state['inst']['classes']['person']['tp'] == 8 and state['inst']['categories']['vehicle']['tp'] == 0
  assert state['inst']['categories']['human']['tp'] == 8 and sc['classInstScores']['person'] == 1.0
  assert all(r['tp'] == 0 for n, r in state['inst']['classes'].items() if n != 'person')
  # the vehicle category counts a caravan prediction on a car instance (generateInstanceStats lists 29 and 30)
  g5, i5, p5 = np.full((2, 4), 26), np.full((2, 4), 26001), np.full((2, 4), 29)
  state, _ = po.evaluate([p5], [g5], [i5])
  assert state['inst']['classes']['car']['tp'] == 0 and state['inst']['categories']['vehicle']['tp'] == 8


def test_label_table_matches_the_other_tables():
  assert [r[0] for r in analysis.PIXEL_LABEL_TABLE] == list(range(34)) == sorted(po.LABELS)
  for lid, name, cat, has, ign in analysis.PIXEL_LABEL_TABLE:
    assert (name, cat, int(has), int(ign)) == po.LABELS[lid]
  assert tuple(r[0] for r in analysis.PIXEL_LABEL_TABLE if r[4]) == analysis.AP_VOID_LABEL_IDS
  assert [(r[1], r[0]) for r in analysis.PIXEL_LABEL_TABLE if r[3] and not r[4]] == analysis.CITYSCAPES_LABELS
  assert analysis.PIXEL_AVG_CLASS_SIZE == po.AVG_CLASS_SIZE and list(analysis.PIXEL_CATEGORIES) == po.CATEGORIES
  assert [l for _, l in analysis.CITYSCAPES_LABELS] == po.THING_LABELS
  assert ops.PIXEL_LABELS == 34 and rn.RA_PIXEL_TILE == ops.PIXEL_TILE


@pytest.mark.parametrize('seed', range(6))
def test_scores_equal_the_oracle_on_random_records(seed):
  rng = np.random.RandomState(seed)
  conf = rng.randint(0, 1 << 40, (34, 34)).astype(np.int64) * (rng.rand(34, 34) > (0.3 if seed else 0.97))
  if seed == 1:
    conf[:] = 0
  if seed == 2:
    conf[24:] = 0
    conf[:, 24:] = 0
  ref, got = po.new_instance_stats(), analysis.pixel_instance_stats()
  assert {c: r['labelIds'] for c, r in got['categories'].items()} == {'human': [24, 25], 'vehicle': [26, 27, 28, 29, 30, 31, 32, 33]}
  assert ref == got
  for _ in range(0 if seed in (1, 2) else 5):  # images
    ids = np.unique(np.concatenate([rng.randint(0, 34, 6), [1000, 24000, 29001], rng.randint(24, 34, 20) * 1000 + rng.randint(0, 40, 20)]))
    size = rng.randint(1, 200000, ids.size)
    tp = (size * rng.rand(ids.size)).astype(np.int64)
    cat_tp = tp + ((size - tp) * rng.rand(ids.size)).astype(np.int64)
    analysis.pixel_instance_stats_add(got, ids, size, tp, cat_tp)
    for i, s, t, c in zip(ids, size, tp, cat_tp):  # :581-615 on the counts
      name, cat, _, ign = po.LABELS[int(i) // 1000]
      if i <= 1000 or ign:
        continue
      w = po.AVG_CLASS_SIZE[name] / float(s)
      for rec, n in ((ref['classes'][name], int(t)), (ref['categories'][cat], int(c))):
        rec['tp'] += n
        rec['fn'] += int(s) - n
        rec['tpWeighted'] += float(n) * w
        rec['fnWeighted'] += float(int(s) - n) * w
  assert ref == got  # the integer sums and, built in the same order, the float64 ones
  a, b = analysis.cityscapes_pixel_scores(conf, got), po.scores(conf, ref)
  po.same_scores(a, b, rel=1e-12)
  res = analysis.cityscapes_pixel_result(conf, got)
  assert res['confMatrix'] == conf.tolist() and res['labels'] == {v[0]: k for k, v in po.LABELS.items()}
  if conf.sum():
    assert res['priors']['road'] == float(conf[7].sum()) / conf.sum()
  thing = {n: b['classScores'][n] for n in ('person', 'rider', 'car', 'truck', 'bus', 'train', 'motorcycle', 'bicycle')}
  x, y = res['averageScorePredictedClasses'], po.average(thing)
  assert (math.isnan(x) and math.isnan(y)) or abs(x - y) <= 1e-12 * abs(y)


def test_scores_on_the_hand_image_and_json_keys(tmp_path, capsys):
  pred, gt, ids = _hand_image()
  state, sc = po.evaluate([pred], [gt], [ids])
  stats = analysis.pixel_instance_stats()
  rows = po.instance_counts(pred, ids)
  analysis.pixel_instance_stats_add(stats, *[[r[k] for r in rows] for k in range(4)])
  assert stats == state['inst']
  po.same_scores(analysis.cityscapes_pixel_scores(state['conf'], stats), sc, rel=0.0)
  an = analysis.CityscapesPixelAnalyzer(['a'])
  an.conf, an.inst_stats, an.pixels = torch.from_numpy(state['conf'].copy()), stats, 24
  path = str(tmp_path / 'resultPixelLevelSemanticLabeling.json')
  res = an.finalize(path)
  with open(path) as f:
    disk = json.load(f)
  assert sorted(disk) == sorted(['confMatrix', 'priors', 'labels'] + po.SCORE_KEYS + po.AVERAGE_KEYS + ['averageScorePredictedClasses'])
  assert disk['classScores']['road'] == 6 / 9.0 and math.isnan(disk['classScores']['sky']) and disk['labels']['bicycle'] == 33
  assert res['averageScorePredictedClasses'] == (3 / 8.0 + 0.0 + 6 / 10.0) / 3  # person, rider, car; the others NaN
  text = capsys.readouterr().out
  assert 'person        : 0.375' in text and 'Score Average' in text and 'vehicle' in text
  an.pixels = 25
  with pytest.raises(rn.RecAttendError, match='disagree'):
    an.finalize()


def test_command_line_pairs_files_by_the_toolkit_rule(tmp_path):
  pred, gt, ids = _hand_image()
  gdir, pdir = tmp_path / 'gt' / 'aachen', tmp_path / 'pred'
  os.makedirs(str(gdir))
  os.makedirs(str(pdir / 'run'))
  stems = ['aachen_000001_000019', 'aachen_000000_000019']
  for s in stems:
    (gdir / (s + '_gtFine_labelIds.png')).write_bytes(po.encode_png(gt, 8))
    (gdir / (s + '_gtFine_instanceIds.png')).write_bytes(po.encode_png(ids, 16))
    (pdir / 'run' / (s + '_pred.png')).write_bytes(po.encode_png(pred, 8))
  gts = cityscapes_pixel.list_ground_truth(str(tmp_path / 'gt'))
  assert [os.path.basename(n) for n, _ in gts] == [s + '_gtFine_labelIds.png' for s in sorted(stems)]
  got_ids, got_labels = gts[0][1]()
  assert got_ids.dtype == np.int32 and (got_ids == ids).all() and got_labels.dtype == np.uint8 and (got_labels == gt).all()
  walk = [(root, files) for root, _, files in os.walk(str(pdir))]
  assert cityscapes_pixel.find_prediction(walk, gts[0][0]) == str(pdir / 'run' / (sorted(stems)[0] + '_pred.png'))
  with pytest.raises(rn.RecAttendError, match='Found no prediction'):
    cityscapes_pixel.find_prediction(walk, 'bonn_000001_000019_gtFine_labelIds.png')
  (pdir / (stems[0] + '_other.png')).write_bytes(po.encode_png(pred, 8))
  with pytest.raises(rn.RecAttendError, match='multiple predictions'):
    cityscapes_pixel.find_prediction([(root, files) for root, _, files in os.walk(str(pdir))], gts[1][0])
  os.remove(str(pdir / (stems[0] + '_other.png')))
  # unequal sizes: an error that names the file, raised before a device is asked for
  (pdir / 'run' / (stems[1] + '_pred.png')).write_bytes(po.encode_png(pred[:, :5], 8))
  with pytest.raises(rn.RecAttendError, match=stems[1] + '_pred.png'):
    cityscapes_pixel.main(['--pred', str(pdir), '--gt', str(tmp_path / 'gt')])
  # the .npz form of --gt
  npz = str(tmp_path / 'gt.npz')
  np.savez(npz, gt_instance_ids=np.stack([ids, ids]).astype(np.int32), names=np.array([s + '.png' for s in stems]))
  got = cityscapes_pixel.list_ground_truth(npz)
  assert [n for n, _ in got] == [s + '.png' for s in stems] and got[0][1]()[1] is None
  np.savez(npz, gt_instance_ids=np.stack([ids, ids]).astype(np.int32), gt_label_ids=np.stack([gt, gt]).astype(np.uint8),
           names=np.array(stems))
  assert (cityscapes_pixel.list_ground_truth(npz)[1][1]()[1] == gt).all()
  np.savez(npz, gt_instance_ids=np.stack([ids, ids]).astype(np.int32))
  with pytest.raises(rn.RecAttendError, match='lacks names'):
    cityscapes_pixel.list_ground_truth(npz)
  os.remove(str(gdir / (stems[0] + '_gtFine_instanceIds.png')))
  with pytest.raises(rn.RecAttendError, match='instanceIds'):
    cityscapes_pixel.list_ground_truth(str(tmp_path / 'gt'))[1][1]()


def test_refusals_need_no_device(monkeypatch):
  def no_lib():
    raise AssertionError('the library was asked for')
  monkeypatch.setattr(rn, 'lib', no_lib)
  u8 = torch.zeros((2, 4, 6), dtype=torch.uint8)
  i32 = torch.zeros((2, 4, 6), dtype=torch.int32)
  sem = torch.zeros((2, 2, 3, 9), dtype=torch.float32)
  for call in (lambda: ops.pixel_confusion(u8, i32), lambda: ops.pixel_confusion(sem, i32, size=(4, 6)), lambda: ops.sem_labels(sem, (4, 6))):
    with pytest.raises(rn.RecAttendError, match='CPU tensor'):
      call()

  class OnDevice(torch.Tensor):
    """A host tensor that says it is on the device, so the refusals behind the first one are reached without a GPU."""
    is_cuda = property(lambda self: True)

  FakeDev = lambda t: t.as_subclass(OnDevice)
  strided = torch.zeros((2, 4, 12), dtype=torch.int32)[:, :, ::2]
  bad = [
      (lambda: ops.sem_labels(FakeDev(sem.double()), (4, 6)), 'float32'),
      (lambda: ops.sem_labels(FakeDev(sem.transpose(1, 2)), (4, 6)), 'contiguous'),
      (lambda: ops.sem_labels(FakeDev(sem), None), 'size'),
      (lambda: ops.sem_labels(FakeDev(torch.zeros((2, 2, 3, 1))), (4, 6)), '2 <= C <= 9'),
      (lambda: ops.sem_labels(FakeDev(torch.zeros((1, 2, 3, 10))), (4, 6)), '2 <= C <= 9'),
      (lambda: ops.sem_labels(FakeDev(sem), (0, 6)), 'planes'),
      (lambda: ops.sem_labels(FakeDev(sem), (1 << 16, 1 << 15)), 'planes'),
      (lambda: ops.pixel_confusion(FakeDev(u8.to(torch.int32)), FakeDev(i32)), 'uint8'),
      (lambda: ops.pixel_confusion(FakeDev(u8[0]), FakeDev(i32)), r'\[B,H,W\]'),
      (lambda: ops.pixel_confusion(FakeDev(u8), FakeDev(i32), size=(4, 7)), 'does not match'),
      (lambda: ops.pixel_confusion(FakeDev(u8), FakeDev(i32.long())), 'int32'),
      (lambda: ops.pixel_confusion(FakeDev(u8), FakeDev(strided)), 'contiguous'),
      (lambda: ops.pixel_confusion(FakeDev(u8), FakeDev(torch.zeros((2, 3, 6), dtype=torch.int32))), 'do not belong together'),
      (lambda: ops.pixel_confusion(FakeDev(u8), FakeDev(i32), FakeDev(i32)), 'gt_labels must be a uint8'),
      (lambda: ops.pixel_confusion(FakeDev(u8), FakeDev(i32), FakeDev(u8[:1])), 'do not belong together'),
      (lambda: ops.pixel_confusion(FakeDev(sem), FakeDev(i32)), 'size'),
      (lambda: ops.pixel_confusion(FakeDev(sem), FakeDev(i32), size=(4, 5)), 'do not belong together'),
      (lambda: ops.pixel_confusion(FakeDev(u8), FakeDev(i32), conf=FakeDev(torch.zeros((34, 34), dtype=torch.int32))), 'int64'),
      (lambda: ops.pixel_confusion(FakeDev(u8), FakeDev(i32), conf=FakeDev(torch.zeros((34, 33), dtype=torch.int64))), r'\[34,34\]'),
      (lambda: ops.pixel_confusion(FakeDev(u8), FakeDev(i32), names=['a']), 'names'),
      (lambda: ops.pixel_confusion(FakeDev(u8), FakeDev(i32), catalog=(FakeDev(torch.zeros((2, 255), dtype=torch.int32)), None,
                                                                       FakeDev(torch.zeros((2,), dtype=torch.int32)))), 'do not belong together'),
      (lambda: ops.pixel_confusion(FakeDev(u8), FakeDev(i32), catalog=(FakeDev(torch.zeros((2, 256))), None,
                                                                       FakeDev(torch.zeros((2,), dtype=torch.int32)))), 'int32'),
  ]
  for call, why in bad:
    with pytest.raises(rn.RecAttendError, match=why):
      call()
  with pytest.raises(rn.RecAttendError, match='label 40'):
    analysis.pixel_instance_stats_add(analysis.pixel_instance_stats(), [40001], [5], [0], [0])
