"""The label stage without a device: the float64 oracle (tests/labels_oracle.py) pinned on cases derived by hand, the C
ABI's argument checks, and the command line of setup_labels.py."""
import os

import numpy as np
import pytest

import labels_oracle as lo
import ra_native as rn


# ---- the oracle on hand-derived cases
def _sector_class(dy, dx):
  """The orientation class of the offset (dy, dx) from the centroid, from the sector boundaries: the folded angle is
  atan2(dy, dx), class k covers atan2 + pi in [(k - 1/2) pi / 4, (k + 1/2) pi / 4), so the boundaries lie at |dy| / |dx| =
  tan(pi / 8) = sqrt(2) - 1 and its inverse — |dy| < (sqrt(2) - 1) |dx| <=> (|dy| + |dx|)^2 < 2 dx^2, in integers.  A zero
  component counts as positive (the + 1e-8 of orientation.py:60), which sends the centroid itself to class 4."""
  ay, ax = abs(dy), abs(dx)
  if (ay + ax) ** 2 < 2 * ax * ax or (ay == 0 and ax == 0):
    return 4 if dx >= 0 else 0
  if (ay + ax) ** 2 < 2 * ay * ay:
    return 6 if dy >= 0 else 2
  return {(False, False): 1, (False, True): 3, (True, True): 5, (True, False): 7}[(dy > 0, dx > 0)]


def test_oracle_orientation_of_a_square():
  img = np.zeros((17, 17), np.int32)
  img[2:15, 2:15] = 3
  got = lo.assemble_image(img, 17, 17, 1, lo.PLAIN)
  want = np.zeros((17, 17), np.uint8)
  for r in range(2, 15):
    for c in range(2, 15):
      want[r, c] = _sector_class(r - 8, c - 8)
  assert np.array_equal(got['d_cls'], want)
  # two rows written out: the top row of the square, and the centroid's (class 0 left of it, shared with the background)
  assert got['d_cls'][2].tolist() == [0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 2, 3, 3, 3, 3, 0, 0]
  assert got['d_cls'][8].tolist() == [0, 0, 0, 0, 0, 0, 0, 0, 4, 4, 4, 4, 4, 4, 4, 0, 0]
  assert got['d_cls'][8, 8] == 4 and got['ori_margin'] > 1e-2
  assert np.array_equal(got['d_gt'].argmax(axis=-1), want) and (got['d_gt'].sum(axis=-1) == 1).all()
  assert got['d_gt'][0, 0].tolist() == [1, 0, 0, 0, 0, 0, 0, 0]  # the background is class 0
  assert got['area'].tolist() == [169] and got['inst_id'].tolist() == [3] and got['s_gt'].tolist() == [1.0]


def test_oracle_sort_and_tie_rule():
  img = np.zeros((8, 8), np.int32)
  img[0, 0:6] = 5    # area 6
  img[2:4, 0:5] = 2  # area 10
  img[5, 1:7] = 9    # area 6: ties with id 5, and the larger catalogue index goes first
  got = lo.assemble_image(img, 8, 8, 4, lo.PLAIN)
  assert got['inst_id'].tolist() == [2, 9, 5, -1] and got['area'].tolist() == [10, 6, 6, 0]
  assert got['s_gt'].tolist() == [1, 1, 1, 0] and got['num_obj'] == 3 and got['sem_cls'].tolist() == [0, 0, 0, -1]
  assert np.array_equal(got['y_gt'][1], (img == 9).astype(np.float32)) and not got['y_gt'][3].any()
  cut = lo.assemble_image(img, 8, 8, 2, lo.PLAIN)  # truncation: s_gt all 1, the orientation still over all three
  assert cut['inst_id'].tolist() == [2, 9] and cut['s_gt'].tolist() == [1, 1] and np.array_equal(cut['d_cls'], got['d_cls'])
  assert np.array_equal(got['c_gt'][..., 0], (img > 0).astype(np.float32)) and np.array_equal(got['fg_gt_full'], (img > 0).astype(np.uint8))


CS_IDS = (7, 24000, 24001, 26003, 29001, 33002, 1000)


def cityscapes_id_image(Hf=14, Wf=12):
  """Every id of CS_IDS as a 2-row band of an image that is background elsewhere."""
  img = np.zeros((Hf, Wf), np.int32)
  for k, ident in enumerate(CS_IDS):
    img[2 * k:2 * k + 2, 1:1 + 3 + k] = ident
  return img


def test_oracle_cityscapes_rule():
  img = cityscapes_id_image()
  got = lo.assemble_image(img, 14, 12, 6, lo.CITYSCAPES)
  # accepted: person 24000, 24001 (class 0), car 26003 (2), bicycle 33002 (7); the stuff id 7, the caravan 29001 and 1000
  # (not > 1000) are background
  assert got['num_obj'] == 4 and got['inst_id'].tolist() == [33002, 26003, 24001, 24000, -1, -1]
  assert got['sem_cls'].tolist() == [7, 2, 0, 0, -1, -1] and got['area'].tolist() == [16, 12, 10, 8, 0, 0]
  assert got['c_gt'].shape == (14, 12, 9) and (got['c_gt'].sum(axis=-1) == 1).all()
  assert np.array_equal(got['c_gt'][..., 1], np.isin(img, (24000, 24001)).astype(np.float32))
  assert np.array_equal(got['c_gt'][..., 3], (img == 26003).astype(np.float32)) and not got['c_gt'][..., 2].any()
  assert np.array_equal(got['c_gt'][..., 0], 1 - np.isin(img, (24000, 24001, 26003, 33002)).astype(np.float32))
  assert np.array_equal(got['fg_gt_full'], np.isin(img, (24000, 24001, 26003, 33002)).astype(np.uint8))
  plain = lo.assemble_image(img, 14, 12, 8, lo.PLAIN)
  assert plain['num_obj'] == 7 and plain['c_gt'].shape == (14, 12, 1)


def test_oracle_nearest_neighbour_rule_and_vanishing_instance():
  assert lo.nn_index(12, 30).tolist() == [0, 2, 5, 7, 10, 12, 15, 17, 20, 22, 25, 27]  # floor(d * 2.5)
  assert lo.nn_index(4, 4).tolist() == [0, 1, 2, 3] and lo.nn_index(3, 7).max() <= 6
  img = np.zeros((8, 8), np.int32)
  img[3, 5] = 4  # odd row and column: not sampled at ratio 2
  got = lo.assemble_image(img, 4, 4, 2, lo.PLAIN)
  assert got['num_obj'] == 1 and got['s_gt'].tolist() == [1, 0] and got['inst_id'].tolist() == [4, -1]
  assert got['area'].tolist() == [0, 0] and not got['y_gt'].any() and not got['d_cls'].any() and got['fg_gt_full'].sum() == 1


def test_binding_shares_the_label_tuple():
  import analysis
  import cs_oracle as co
  import ra_ops as ops
  assert analysis.CITYSCAPES_LABELS == co.LABELS == lo.LABELS and len(ops._cityscapes_labels()) == 8
  assert (rn.RA_LABELS_PLAIN, rn.RA_LABELS_CITYSCAPES, rn.RA_LABELS_MAX_T) == (0, 1, 32)
  assert ops.label_dataset_rule('kitti') == ops.label_dataset_rule('cvppp') == rn.RA_LABELS_PLAIN
  assert ops.label_dataset_rule('cityscapes') == ops.label_dataset_rule(rn.RA_LABELS_CITYSCAPES) == rn.RA_LABELS_CITYSCAPES
  with pytest.raises(rn.RecAttendError, match='dataset'):
    ops.label_dataset_rule('mscoco_person')


# ---- the C ABI's argument checks
def test_argument_validation_without_gpu():
  lib = rn.lib()
  one = 16  # any non-null address: the shape is refused before anything is read or launched
  call = lambda T, H, W, dataset=0, ws=one, Hf=8, Wf=8: lib.ra_labels_assemble_i32(
      one, one, one, 1, Hf, Wf, H, W, T, dataset, ws, 1 << 30, one, one, one, one, one, one, one, one, one, one, None)
  for T, H, W in ((0, 4, 4), (33, 4, 4), (2, 9, 4), (2, 4, 9), (2, 0, 4), (2, 4, 0)):
    assert call(T, H, W) == rn.RA_E_SHAPE and b'ra_labels_assemble_i32' in lib.ra_last_error_string()
  assert call(2, 4, 4, dataset=2) == rn.RA_E_SHAPE
  assert call(2, 4, 4, Hf=1 << 16, Wf=1 << 15) == rn.RA_E_SHAPE  # Hf * Wf = 2^31
  assert call(2, 4, 4, ws=None) == rn.RA_E_INVALID
  assert lib.ra_labels_assemble_i32(None, one, one, 1, 8, 8, 4, 4, 2, 0, one, 1 << 30, *([None] * 10), None) == rn.RA_E_INVALID
  assert lib.ra_labels_assemble_i32(one, one, one, 1, 8, 8, 4, 4, 2, 0, one, 8, *([one] * 10), None) == rn.RA_E_WORKSPACE
  # one workgroup's three 64-bit counters per slot, the two centroid coordinates and the rank table
  assert lib.ra_labels_workspace_bytes(1, 8, 8) == 256 * (3 * 8 + 2 * 8 + 4)
  assert lib.ra_labels_workspace_bytes(8, 256, 512) == 8 * (64 * 3 * 256 * 8 + 256 * 20)
  assert lib.ra_labels_workspace_bytes(0, 8, 8) == 0


def test_no_device_raises(monkeypatch):
  import torch
  import ra_ops as ops
  monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
  with pytest.raises(rn.RecAttendError, match='no CPU fallback'):
    ops.assemble_labels(np.zeros((1, 8, 8), np.int32), 4, 4, 2, 'cvppp')
  with pytest.raises(rn.RecAttendError, match='no CPU fallback'):
    ops.assemble_labels(torch.zeros((1, 8, 8), dtype=torch.int32), 4, 4, 2, 'cvppp')
  with pytest.raises(rn.RecAttendError, match='integers'):
    ops.assemble_labels(np.zeros((1, 8, 8), np.float32), 4, 4, 2, 'cvppp')


# ---- the command line
def _archive(tmp_path, with_x=True):
  rng = np.random.RandomState(0)
  ids = lo.ellipse_ids(rng, 2, 16, 24, 3)
  src = str(tmp_path / 'ids.npz')
  extra = {'x': rng.rand(2, 8, 12, 3).astype(np.float32)} if with_x else {}
  np.savez(src, gt_instance_ids=ids, names=np.array(['a.png', 'b.png']), **extra)
  return src, ids


def test_command_line_argument_errors(tmp_path, monkeypatch):
  import torch
  import setup_labels as sl
  from utils import png
  src, ids = _archive(tmp_path)
  out = str(tmp_path / 'out.npz')
  for argv in (['--input', src, '--output', out], ['--input', src, '--dataset', 'mscoco', '--output', out],
               ['--input', src, '--dataset', 'kitti', '--target', 'box', '--output', out], ['--dataset', 'kitti', '--output', out]):
    with pytest.raises(SystemExit):
      sl.main(argv)
  size = ['--height', '8', '--width', '12', '--timespan', '4']
  np.savez(str(tmp_path / 'bad.npz'), x=np.zeros((1, 2, 2, 3), np.float32))
  with pytest.raises(rn.RecAttendError, match='lacks gt_instance_ids'):
    sl.main(['--input', str(tmp_path / 'bad.npz'), '--dataset', 'kitti', '--output', out] + size)
  with pytest.raises(rn.RecAttendError, match='timespan'):
    sl.main(['--input', src, '--dataset', 'kitti', '--output', out, '--height', '8', '--width', '12', '--timespan', '33'])
  with pytest.raises(rn.RecAttendError, match='no larger than the labels'):
    sl.main(['--input', src, '--dataset', 'kitti', '--output', out])  # KITTI's 128 x 448 from labels of 16 x 24
  with pytest.raises(rn.RecAttendError, match='network size'):
    sl.main(['--input', src, '--dataset', 'kitti', '--output', out, '--height', '4', '--width', '12', '--timespan', '4'])  # x is 8 x 12
  # a folder: grey 8- and 16-bit files are read, a colour file and mixed sizes are refused
  folder = tmp_path / 'png'
  os.makedirs(str(folder / 'sub'))
  png.write_gray8(str(folder / 'sub' / 'b.png'), ids[1].astype(np.uint8))
  png.write_gray8(str(folder / 'a.png'), ids[0].astype(np.uint8))
  got, names, x = sl.load_input(str(folder))
  assert names == ['a.png', 'b.png'] and x is None and np.array_equal(got, ids) and got.dtype == np.int32
  with open(str(folder / 'a.png'), 'rb') as f:
    data = bytearray(f.read())
  data[25] = 2  # colour type RGB
  with open(str(folder / 'c.png'), 'wb') as f:
    f.write(bytes(data))
  with pytest.raises(rn.RecAttendError, match='colour type 2'):
    sl.load_input(str(folder))
  os.remove(str(folder / 'c.png'))
  png.write_gray8(str(folder / 'd.png'), np.zeros((3, 3), np.uint8))
  with pytest.raises(rn.RecAttendError, match='different sizes'):
    sl.load_input(str(folder))
  os.makedirs(str(tmp_path / 'empty'))
  with pytest.raises(rn.RecAttendError, match=r'no \*\.png'):
    sl.load_input(str(tmp_path / 'empty'))
  monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
  with pytest.raises(rn.RecAttendError, match='no CPU fallback'):
    sl.main(['--input', src, '--dataset', 'kitti', '--output', out] + size)
  assert not os.path.exists(out)


@pytest.mark.parametrize('target,dataset,keys', [
    ('full_model', 'cvppp', {'y_gt', 's_gt', 'x'}),
    ('fg_model', 'cityscapes', {'y_gt', 'd_gt', 'fg_gt_full', 'names', 'x'}),
    ('all', 'kitti', {'y_gt_ins', 's_gt', 'c_gt', 'd_gt', 'd_cls', 'fg_gt_full', 'inst_id', 'area', 'sem_cls', 'num_obj', 'names', 'x'}),
])
def test_command_line_key_sets(tmp_path, monkeypatch, target, dataset, keys):
  """What setup_labels.py writes per --target, with the device op replaced by the oracle: the archive's keys, shapes and
  the renaming (fg_model's y_gt is the semantic map c_gt); the op itself is tests/test_labels_gpu.py's."""
  import torch
  import ra_ops as ops
  import setup_labels as sl
  src, ids = _archive(tmp_path)
  calls = []

  def fake(gt_ids, H, W, T, ds, want=(), names=None):
    calls.append((tuple(gt_ids.shape), ds, tuple(want), list(names)))
    ref = lo.assemble(gt_ids, H, W, T, lo.CITYSCAPES if ds == 'cityscapes' else lo.PLAIN)
    return {k: torch.from_numpy(np.ascontiguousarray(ref[k])) for k in want}

  monkeypatch.setattr(ops, 'assemble_labels', fake)
  monkeypatch.setattr(torch.cuda, 'is_available', lambda: True)
  out = str(tmp_path / 'o' / 'out.npz')
  sl.main(['--input', src, '--dataset', dataset, '--height', '8', '--width', '12', '--timespan', '4', '--target', target,
           '--output', out, '--batch_size', '1'])
  got = dict(np.load(out))
  assert set(got) == keys and len(calls) == 2 and calls[0][0] == (1, 16, 24) and calls[1][3] == ['b.png']
  ref = lo.assemble(ids, 8, 12, 4, lo.CITYSCAPES if dataset == 'cityscapes' else lo.PLAIN)
  if target == 'full_model':
    assert np.array_equal(got['y_gt'], ref['y_gt']) and got['y_gt'].shape == (2, 4, 8, 12) and got['s_gt'].shape == (2, 4)
  elif target == 'fg_model':
    assert np.array_equal(got['y_gt'], ref['c_gt']) and got['y_gt'].shape == (2, 8, 12, 9) and got['d_gt'].shape == (2, 8, 12, 8)
    assert got['fg_gt_full'].dtype == np.uint8 and got['fg_gt_full'].shape == (2, 16, 24) and got['names'].tolist() == ['a.png', 'b.png']
  else:
    assert np.array_equal(got['y_gt_ins'], ref['y_gt']) and got['c_gt'].shape == (2, 8, 12, 1) and got['d_cls'].dtype == np.uint8
    assert np.array_equal(got['num_obj'], ref['num_obj']) and got['num_obj'].max() <= 3
  assert got['x'].shape == (2, 8, 12, 3)
  assert set(sl.TARGETS) == {'full_model', 'fg_model', 'all'}
