"""The Cityscapes output stage behind a label-image segmentation, without a GPU: the integer oracle (tests/label_vote_oracle.py)
against the float64 restatement of the stage (tests/cs_oracle.py) fed the one-hot map, the three LUTs, the command line, the
label-image reader's errors, the header's new symbols and the refusals the library makes before any launch."""
import ctypes as C

import numpy as np
import pytest

import cs_oracle as co
import label_vote_oracle as lo
import ra_native as rn
import ra_oracle as ora

THRESHOLDS = [0.0, 0.25, 0.5, 0.75, 0.0]   # exact in float32; the last one again: sizes recover, conf does not
REMOVE_TINY = 10
SCORES = [0.9, 0.8, 0.7, 0.95, 0.85, 0.5]


def hand_scene():
  """B = 1, T = 6, 32 x 64 (powers of two: the reference's float means are exact).  Values are the masks AFTER
  apply_confidence, on a grid of 1 / 64.  Instance 0: a large car.  1: 24 pixels at 0.3125 and 6 at 0.875 on a person — kept
  up to 0.25, tiny from 0.5 on.  2: 20 pixels of person, 12 of rider.  3: 15 of bus (met first in raster order) and 15 of
  truck: a tie.  4: 20 pixels of car, 10 of road.  5: score exactly 0.5.  Seeded noise below 0.2 in every plane."""
  rng = np.random.RandomState(11)
  B, T, H, W = 1, 6, 32, 64
  y = (rng.randint(0, 12, (B, T, H, W)) / 64.0).astype(np.float32)
  y[rng.rand(B, T, H, W) < 0.5] = 0.0
  labels = np.full((B, H, W), 7, np.uint8)                         # road
  labels[0, :, 60:] = 255
  labels[0, 2:14, 2:22] = 26;   y[0, 0, 2:14, 2:22] = 0.90625      # instance 0: 240 pixels of car
  labels[0, 16:21, 2:8] = 24
  y[0, 1, 16:20, 2:8] = 0.3125;  y[0, 1, 20, 2:8] = 0.875          # instance 1: 24 + 6 on a person
  labels[0, 16:20, 12:17] = 24;  labels[0, 16:20, 17:20] = 25
  y[0, 2, 16:20, 12:20] = 0.78125                                  # instance 2: 20 person + 12 rider
  labels[0, 24:27, 2:7] = 28;    labels[0, 27:30, 2:7] = 27
  y[0, 3, 24:30, 2:7] = 0.953125                                   # instance 3: 15 bus, then 15 truck
  labels[0, 24:28, 12:17] = 26
  y[0, 4, 24:28, 12:17] = 0.84375;  y[0, 4, 28:30, 12:17] = 0.84375  # instance 4: 20 on car, 10 on road
  labels[0, 2:8, 30:40] = 33;    y[0, 5, 2:8, 30:40] = 0.796875    # instance 5: 60 pixels of bicycle, score 0.5
  return y, labels, np.array([SCORES], np.float32)


def test_oracle_agrees_with_the_float64_stage_on_the_one_hot_map():
  y, labels, s = hand_scene()
  lut = lo.class_lut('labelIds')
  got = lo.sweep(y, labels, lut, THRESHOLDS, s, REMOVE_TINY)
  oh = lo.onehot(labels, lut)
  one = ora.pp_apply_one_label(y.astype(np.float64))
  ref = co.threshold_chain(one, 1 - oh[..., 0], oh, s.astype(np.float64), THRESHOLDS, REMOVE_TINY)
  for k, r in enumerate(ref):
    assert np.array_equal(got['label_id'][k], r['label_id']) and np.array_equal(got['class_idx'][k], r['class_idx'])
    assert np.array_equal(got['conf'][k].astype(np.float64), r['conf'])
    assert np.array_equal(got['sizes'][k], r['sizes'])
    assert np.abs(got['vote'][k].astype(np.float64) - r['vote']).max() <= 1e-12
    assert np.array_equal(lo.planes(y, labels, lut, THRESHOLDS[k], got['keep'][k]), r['y_out'].astype(np.float32))

  # the cases, asserted on the oracle's own output
  sizes, conf, cnt, idx, lab = got['sizes'][:, 0], got['conf'][:, 0], got['counts'][:, 0], got['class_idx'][:, 0], got['label_id'][:, 0]
  # kept at the first thresholds, dropped by remove_tiny at 0.5: conf is zero from then on, also where the size recovers
  assert sizes[0, 1] > REMOVE_TINY and sizes[1, 1] > REMOVE_TINY and got['keep'][:2, 0, 1].all() and conf[1, 1] == np.float32(0.8)
  assert sizes[2, 1] == 6 and not got['keep'][2, 0, 1] and (conf[2:, 1] == 0).all() and (idx[2:, 1] == -1).all()
  assert sizes[4, 1] > REMOVE_TINY and got['keep'][4, 0, 1] and conf[4, 1] == 0 and got['vote'][4, 0, 1].sum() > 0
  # over two thing classes with different counts
  assert cnt[2, 2, 0] == 20 and cnt[2, 2, 1] == 12 and lab[2, 2] == 24
  # an exact tie of two class counts: the first class wins
  assert cnt[3, 3, 3] == cnt[3, 3, 4] == 15 and idx[3, 3] == 3 and lab[3, 3] == 27
  # masked background pixels under a mask
  am, v = lo.one_label(y)
  under = (am[0] == 4) & (v[0] > 0.5)
  assert under.sum() == 30 and (lut[labels[0]][under] == 0).sum() == 10 and sizes[2, 4] == 20
  # a score of exactly 0.5 is not written, at any threshold
  assert (conf[:, 5] == 0.5).all() and (idx[:, 5] == -1).all() and (lab[:, 5] == -1).all() and sizes[3, 5] == 60
  assert lo.text_lines('a_b_c.png', conf[3], lab[3], idx[3]) == [
      ('a_b_c_000.png', 26, float(np.float32(0.9))), ('a_b_c_002.png', 24, float(np.float32(0.7))),
      ('a_b_c_003.png', 27, float(np.float32(0.95))), ('a_b_c_004.png', 26, float(np.float32(0.85)))]


def test_oracle_threshold_is_strict_in_float32_and_order_free():
  f = np.float32(0.3)
  y = np.array([f, np.nextafter(f, np.float32(1)), 0.0, -0.5], np.float32).reshape(1, 1, 1, 4)
  labels = np.full((1, 1, 4), 26, np.uint8)
  got = lo.sweep(y, labels, lo.class_lut('labelIds'), [0.3, -0.1, 0.3, -1.0], np.ones((1, 1), np.float32), 0)
  assert got['sizes'][:, 0, 0].tolist() == [1, 3, 1, 4] and got['keep'].all()          # 0.3 itself is excluded, one ulp above is in
  assert got['counts'][1, 0, 0].tolist() == [0, 0, 3, 0, 0, 0, 0, 0] and (got['label_id'] == 26).all()
  assert got['vote'][1, 0, 0, 3] == np.float32(0.75) and got['vote'][..., 0].max() == 0


def test_the_three_luts():
  import ra_ops as ops
  for ids, first in (('labelIds', None), ('trainIds', 11), ('lrr', 12)):
    lut = ops.label_class_lut(ids)
    assert lut.dtype == np.uint8 and lut.shape == (256,) and np.array_equal(lut, lo.class_lut(ids))
    want = [24, 25, 26, 27, 28, 31, 32, 33] if first is None else list(range(first, first + 8))
    assert np.flatnonzero(lut).tolist() == want and lut[want].tolist() == list(range(1, 9))
  assert ops.label_class_lut('labelIds')[[0, 7, 23, 29, 30, 34, 255]].tolist() == [0] * 7    # caravan and trailer are not voted for
  with pytest.raises(rn.RecAttendError, match='ids'):
    ops.label_class_lut('ids')
  assert tuple(ops.LABEL_CLASS_IDS['labelIds']) == lo.LABEL_IDS == tuple(l for _, l in co.LABELS)
  import cityscapes_eval as ce
  assert sorted(ce.SEMANTIC_LABEL_IDS) == sorted(ops.LABEL_CLASS_IDS)   # the parser's choices are the LUTs there are


def test_parser_has_the_flag_and_still_refuses_lrr():
  import cityscapes_eval as ce
  a = ce.build_parser().parse_args([])
  assert a.semantic_labels is None and a.semantic_label_ids == 'labelIds'
  a = ce.build_parser().parse_args(['--semantic_labels', 'seg', '--semantic_label_ids', 'lrr'])
  assert a.semantic_labels == 'seg' and a.semantic_label_ids == 'lrr'
  with pytest.raises(SystemExit):
    ce.build_parser().parse_args(['--semantic_label_ids', 'ids'])
  with pytest.raises(rn.RecAttendError, match='LRR'):
    ce.main(['--lrr_seg', '--semantic_labels', 'seg', '--input', 'nowhere.npz', '--output', 'nowhere'])
  with pytest.raises(rn.RecAttendError, match='--semantic_labels'):
    ce.main(['--lrr_seg', '--input', 'nowhere.npz', '--output', 'nowhere'])


def test_label_image_reader_and_its_errors(tmp_path):
  import cityscapes_eval as ce
  from utils import png
  rng = np.random.RandomState(5)
  imgs = rng.randint(0, 34, (3, 6, 10)).astype(np.uint8)
  names = ['aachen_000001_000019_leftImg8bit.png', 'bonn_000002_000019', 'ulm_000003_000019']
  d = tmp_path / 'seg'
  (d / 'aachen').mkdir(parents=True)
  png.write_gray8(str(d / 'aachen' / 'aachen_000001_000019_pred_labelIds.png'), imgs[0])
  png.write_gray8(str(d / 'bonn_000002_000019.png'), imgs[1])
  read = ce.semantic_label_reader(str(d), names, (6, 10))
  assert np.array_equal(read(0), imgs[0]) and np.array_equal(read(1), imgs[1]) and read(0).dtype == np.uint8
  with pytest.raises(rn.RecAttendError, match='no label image for ulm_000003_000019'):
    read(2)
  png.write_gray8(str(d / 'aachen' / 'aachen_000001_000019_other.png'), imgs[0])
  with pytest.raises(rn.RecAttendError, match='several label images for aachen_000001_000019_leftImg8bit.png'):
    ce.semantic_label_reader(str(d), names, (6, 10))(0)
  with pytest.raises(rn.RecAttendError, match=r'bonn_000002_000019\.png is 6 x 10, expected full_size 12 x 10'):
    ce.semantic_label_reader(str(d), names, (12, 10))(1)
  # the .npz form: any order, by name
  f = str(tmp_path / 'seg.npz')
  np.savez(f, labels=imgs[::-1], names=np.array(names[::-1]))
  read = ce.semantic_label_reader(f, names, (6, 10))
  assert all(np.array_equal(read(i), imgs[i]) for i in range(3))
  with pytest.raises(rn.RecAttendError, match='no label image for paris_1_2'):
    ce.semantic_label_reader(f, ['paris_1_2'], (6, 10))(0)
  with pytest.raises(rn.RecAttendError, match='expected full_size 8 x 10'):
    ce.semantic_label_reader(f, names, (8, 10))(0)
  np.savez(f, labels=imgs[[0, 0]], names=np.array([names[0], names[0]]))
  with pytest.raises(rn.RecAttendError, match='2 times'):
    ce.semantic_label_reader(f, names, (6, 10))(0)
  np.savez(f, labels=imgs.astype(np.int32), names=np.array(names))
  with pytest.raises(rn.RecAttendError, match='uint8'):
    ce.semantic_label_reader(f, names, (6, 10))
  np.savez(f, labels=imgs)
  with pytest.raises(rn.RecAttendError, match='lacks names'):
    ce.semantic_label_reader(f, names, (6, 10))
  with pytest.raises(rn.RecAttendError, match='neither a folder nor'):
    ce.semantic_label_reader(str(tmp_path / 'nothing'), names, (6, 10))


def test_header_symbols_are_bound():
  for name, nargs in (('ra_label_vote_sweep_f32', 19), ('ra_label_planes_f32', 11)):
    assert name in rn.SIGNATURES and len(rn.SIGNATURES[name][1]) == nargs and rn.SIGNATURES[name][0] is C.c_int
    assert getattr(rn.lib(), name).argtypes == rn.SIGNATURES[name][1]
  assert rn.SIGNATURES['ra_label_planes_f32'][1][7] is C.c_double   # thresh: rounded to float32 inside, as the sweep's are


def test_library_refuses_before_any_launch():
  lib = rn.lib()
  one = 16  # any non-null address: the shape is refused before anything is read or launched
  lut = lo.class_lut('labelIds')
  th = np.arange(17, dtype=np.float64) / 20

  def sweep(T=2, K=3, B=1, H=8, W=8, lut=lut, th=th):
    return lib.ra_label_vote_sweep_f32(one, one, rn.ptr(lut), B, T, H, W, rn.ptr(th), K, one, 0, one, one, one, one, one, one,
                                       one, None)
  for kw in ({'T': 33}, {'T': 0}, {'K': 17}, {'K': 0}, {'B': 65536}, {'H': 1 << 15, 'W': (1 << 15) + 1}):
    assert sweep(**kw) == rn.RA_E_SHAPE and b'ra_label_vote_sweep_f32' in lib.ra_last_error_string(), kw
  bad = lut.copy()
  bad[200] = 9
  assert sweep(lut=bad) == rn.RA_E_SHAPE and b'lut[200] = 9' in lib.ra_last_error_string()
  assert lib.ra_label_planes_f32(one, one, rn.ptr(bad), 1, 2, 8, 8, 0.5, None, one, None) == rn.RA_E_SHAPE
  assert lib.ra_label_planes_f32(one, one, rn.ptr(lut), 1, 33, 8, 8, 0.5, None, one, None) == rn.RA_E_SHAPE
  assert b'ra_label_planes_f32' in lib.ra_last_error_string()
  assert lib.ra_label_planes_f32(None, one, rn.ptr(lut), 1, 2, 8, 8, 0.5, None, one, None) == rn.RA_E_INVALID
  assert lib.ra_label_vote_sweep_f32(one, one, None, 1, 2, 8, 8, rn.ptr(th), 3, one, 0, one, one, one, one, one, one, one,
                                     None) == rn.RA_E_INVALID
  nan = np.array([0.1, np.nan])
  assert sweep(K=2, th=nan) == rn.RA_E_INVALID


def test_wrappers_name_the_argument_and_have_no_cpu_path():
  import torch
  import cityscapes_eval as ce
  import ra_ops as ops
  y, labels, s = torch.zeros(1, 2, 8, 8), torch.zeros(1, 8, 8, dtype=torch.uint8), torch.ones(1, 2)
  lut = ops.label_class_lut('labelIds')
  with pytest.raises(rn.RecAttendError, match='label_vote_sweep: y must be a CUDA'):
    ops.label_vote_sweep(y, labels, lut, [0.5], s, 0)
  with pytest.raises(rn.RecAttendError, match='label_planes: y must be a CUDA'):
    ops.label_planes(y, labels, lut, 0.5)
  if not torch.cuda.is_available():
    with pytest.raises(rn.RecAttendError, match='no device is available'):
      list(ce.iter_label_instances_from_labels(y, s, labels, (8, 8), [0.5]))
