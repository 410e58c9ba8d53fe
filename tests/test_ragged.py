"""Mixed full sizes in one batch, without a device: the flat layout (ra_ops.pack_ragged, setup_labels.load_input(...,
mixed_sizes=True)), the conditions on the inputs of tests/test_ragged_gpu.py (the evaluator's and the sweep's bands, the
orientation margin of the label cases), and the new entry points in the header and the binding."""
import ctypes
import os

import numpy as np
import pytest
import torch

import ins_eval_oracle as ieo
import labels_oracle as lo
import ra_native as rn
import ra_ops as ops
import ragged_cases as rc
import setup_labels
from utils import png

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ('ra_gt_instance_catalog_ragged_workspace_ints', 'ra_gt_instance_catalog_ragged_i32', 'ra_labels_assemble_ragged_i32',
                'ra_instance_eval_counts_ragged_f32', 'ra_fg_sweep_counts_ragged_f32')


def test_pack_ragged_layout_and_round_trip():
  rng = np.random.RandomState(3)
  images = [rng.randint(0, 60000, (h, w)).astype(np.int32) for h, w in rc.EVAL_SIZES]
  flat, geo = ops.pack_ragged(images, torch.int32, device='cpu')
  want, total = rc.geometry(rc.EVAL_SIZES, 4)
  assert geo.dtype == np.int64 and np.array_equal(geo, want) and flat.shape == (total,) and flat.dtype == torch.int32
  assert geo[:, 0].tolist() == [0, 1852, 3900, 6096, 6100, 14548] and total == 14548 + 35
  assert not (geo[:, 0] % ops.RAGGED_ALIGN).any()  # every image starts at a multiple of 4 elements
  assert (geo[1:, 0] >= geo[:-1, 0] + geo[:-1, 1] * geo[:-1, 2]).all()  # ascending, no overlap
  back = ops.unpack_ragged(flat, geo)
  covered = np.zeros(total, bool)
  for (off, h, w), img, b in zip(geo.tolist(), images, back):
    assert tuple(b.shape) == (h, w) and np.array_equal(b.numpy(), img)
    assert np.array_equal(flat[off:off + h * w].numpy(), img.reshape(-1))  # rows packed with pitch w
    covered[off:off + h * w] = True
  assert not flat.numpy()[~covered].any()  # the gaps are zero
  tight, g1 = ops.pack_ragged(images, torch.uint8, device='cpu', align=1)
  assert g1[:, 0].tolist() == [0, 1850, 3898, 6091, 6095, 14543] and tight.dtype == torch.uint8
  assert np.array_equal(ops.ragged_geometry(rc.EVAL_SIZES, 1)[0], rc.geometry(rc.EVAL_SIZES, 1)[0])
  with pytest.raises(rn.RecAttendError, match=r'\[h,w\] arrays'):
    ops.pack_ragged([np.zeros((2, 3, 4))], torch.int32, device='cpu')
  with pytest.raises(rn.RecAttendError, match='h, w >= 1'):
    ops.ragged_geometry([(3, 0)])


def test_load_input_mixed_sizes(tmp_path):
  rng = np.random.RandomState(5)
  sizes = {'a.png': (9, 14), 'b.png': (10, 13), 'sub/c.png': (9, 14), 'd.png': (11, 7)}
  imgs = {}
  (tmp_path / 'sub').mkdir()
  for name, (h, w) in sizes.items():
    imgs[name] = rng.randint(0, 200, (h, w)).astype(np.uint8)
    png.write_gray8(str(tmp_path / name), imgs[name])
  with pytest.raises(rn.RecAttendError, match='different sizes'):  # the default is unchanged
    setup_labels.load_input(str(tmp_path))
  flat, names, x = setup_labels.load_input(str(tmp_path), mixed_sizes=True)
  order = ['a.png', 'b.png', 'd.png', 'sub/c.png']  # find_files: sorted by path
  assert names == [os.path.basename(n) for n in order] and x is None
  assert sorted(flat) == ['gt_instance_ids_flat', 'orig_size', 'pixel_offset']
  ids, off, size = flat['gt_instance_ids_flat'], flat['pixel_offset'], flat['orig_size']
  assert ids.dtype == np.int32 and off.dtype == np.int64 and size.dtype == np.int32
  assert size.tolist() == [list(sizes[n]) for n in order]
  assert off.tolist() == [0, 128, 260, 340, 468] and ids.shape == (468,) and not (off % 4).any()
  for i, n in enumerate(order):
    h, w = sizes[n]
    assert np.array_equal(ids[off[i]:off[i] + h * w].reshape(h, w), imgs[n])
  geo = setup_labels.flat_geometry(off, size, 1, 3)
  assert geo.tolist() == [[0, 10, 13], [132, 11, 7]]
  setup_labels.check_flat('here', ids, off, size, 4)
  with pytest.raises(rn.RecAttendError, match='image 1 is 10 x 13 at element 128, the next one starts at 256'):
    bad = off.copy()
    bad[2] = 256
    setup_labels.check_flat('here', ids, bad, size)
  # an archive in the flat format, and one of a single size, load into the same structure
  np.savez(str(tmp_path / 'flat.npz'), names=np.asarray(names), **flat)
  again, names2, _ = setup_labels.load_input(str(tmp_path / 'flat.npz'), mixed_sizes=True)
  assert names2 == names and all(np.array_equal(again[k], flat[k]) for k in flat)
  np.savez(str(tmp_path / 'one.npz'), gt_instance_ids=np.stack([imgs['a.png'], imgs['sub/c.png']]).astype(np.int32))
  one, _, _ = setup_labels.load_input(str(tmp_path / 'one.npz'), mixed_sizes=True)
  assert one['orig_size'].tolist() == [[9, 14], [9, 14]] and one['pixel_offset'].tolist() == [0, 128, 256]
  assert '--mixed_sizes' in setup_labels.build_parser().format_help() and 'reference' in setup_labels.build_parser().format_help()


@pytest.mark.parametrize('morph', [False, True])
@pytest.mark.parametrize('with_fg', [False, True])
def test_the_band_conditions_hold_for_the_ragged_evaluator_cases(morph, with_fg):
  for i in range(len(rc.EVAL_SIZES)):
    c = rc.ins_eval_image(i)
    assert c['gt_ids'].shape == (1,) + rc.EVAL_SIZES[i] and c['yc'].shape == (1, rc.EVAL_T, rc.EVAL_HS, rc.EVAL_WS)
    for K in (1, 10, 16):
      lo_, hi_, share, ties, inter, area_b = rc.ins_eval_reference(i, K, with_fg, morph)
      assert share <= ieo.BAND_SHARE and ties == 0, (i, K, share, ties)
      assert (lo_ <= inter).all() and (inter <= hi_).all()


def test_the_band_condition_holds_for_the_ragged_sweep_cases():
  delta, cap = 1e-5, 1e-3  # tests/test_fg_eval_gpu.py: DELTA, BAND_SHARE
  worst = 0.0
  for i, (h, w) in enumerate(rc.EVAL_SIZES):
    _, _, inside = rc.sweep_band(i, delta)
    assert inside.max() <= 1
    worst = max(worst, inside.max() / float(h * w))
  assert worst <= cap
  print('the worst share of an image inside the band: %.2e' % worst)


@pytest.mark.parametrize('dataset', [lo.PLAIN, lo.CITYSCAPES], ids=['plain', 'cityscapes'])
def test_the_label_cases_keep_the_orientation_margin(dataset):
  for i, (h, w) in enumerate(rc.LABEL_SIZES):
    img, ref = rc.label_image(i, dataset), rc.label_reference(i, dataset)
    assert img.shape == (h, w) and rc.LABEL_H <= h and rc.LABEL_W <= w
    assert ref['ori_margin'] >= 1e-6, (i, ref['ori_margin'])  # tests/test_labels_gpu.py: ORI_GUARD
  assert max(int(rc.label_reference(i, dataset)['num_obj'][0]) for i in range(len(rc.LABEL_SIZES))) >= 2


def test_the_packed_layout_misaligns_the_wide_images():
  geo, _ = rc.geometry(rc.EVAL_SIZES, 1)
  assert geo[1].tolist() == [1850, 16, 128] and geo[1, 0] % 4 == 2 and geo[4, 0] % 4 != 0  # w % 4 == 0, but not the offset
  order, _ = rc.layout('reversed', 6)
  assert order == [5, 4, 3, 2, 1, 0]
  a = np.arange(12).reshape(6, 2)
  assert np.array_equal(rc.unpermute(order, a[order]), a)


def test_entry_points_in_header_and_binding():
  text = open(os.path.join(ROOT, 'include', 'recattend.h')).read()
  lib = ctypes.CDLL(rn.LIB_PATH)
  for name in ENTRY_POINTS:
    assert name + '(' in text and name in rn.SIGNATURES and hasattr(lib, name), name
  assert 'typedef struct ra_image_geo' in text
  assert rn.ImageGeo._fields_ == [('offset', ctypes.c_longlong), ('h', ctypes.c_int), ('w', ctypes.c_int)]
  assert ctypes.sizeof(rn.ImageGeo) == 16 and rn.ImageGeo.offset.offset == 0 and rn.ImageGeo.h.offset == 8 and rn.ImageGeo.w.offset == 12
  P, I, Z = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
  assert rn.SIGNATURES['ra_gt_instance_catalog_ragged_workspace_ints'] == (Z, [P, I])
  assert rn.SIGNATURES['ra_fg_sweep_counts_ragged_f32'] == (I, [P, P, Z, P, P, I, I, I, P, I, P, P])
  assert rn.SIGNATURES['ra_instance_eval_counts_ragged_f32'] == (I, [P, P, P, P, Z, P, P, I, I, I, I, I, P, I, P, P, P])
  for fn in ('gt_instance_catalog_ragged', 'assemble_labels_ragged', 'instance_eval_counts_ragged', 'fg_sweep_counts_ragged', 'pack_ragged'):
    assert callable(getattr(ops, fn))


def test_host_side_refusals_without_a_device():
  """The geometry is checked in host code before anything is launched: the refusals need no GPU."""
  lib = rn.lib()
  tab = (rn.ImageGeo * 2)(rn.ImageGeo(0, 37, 50), rn.ImageGeo(1849, 37, 50))
  thr = np.array([0.3], np.float32)
  one = ctypes.c_void_p(16)  # never dereferenced: the entry refuses first
  rcode = lib.ra_fg_sweep_counts_ragged_f32(one, one, 3700, tab, one, 2, 8, 12, thr.ctypes.data, 1, one, None)
  assert rcode == rn.RA_E_SHAPE and b'image 1 starts at element 1849, inside image 0' in lib.ra_last_error_string()
  tab[1].offset = 1850
  rcode = lib.ra_fg_sweep_counts_ragged_f32(one, one, 3699, tab, one, 2, 8, 12, thr.ctypes.data, 1, one, None)
  assert rcode == rn.RA_E_SHAPE and b'image 1 (37 x 50 at element 1850) ends at 3700, beyond the buffer\'s 3699 elements' in lib.ra_last_error_string()
  tab[0].h = 0
  rcode = lib.ra_gt_instance_catalog_ragged_i32(one, 3700, tab, one, 2, one, 1 << 20, one, one, one, one, None)
  assert rcode == rn.RA_E_SHAPE and b'image 0 is 0 x 50' in lib.ra_last_error_string()
  tab[0].h, tab[1].h, tab[1].w = 37, 4097, 4096
  rcode = lib.ra_instance_eval_counts_ragged_f32(one, one, one, None, 1 << 30, tab, one, 2, 4, 8, 12, 0, thr.ctypes.data, 1, one, one, None)
  assert rcode == rn.RA_E_SHAPE and b'image 1 is 4097 x 4096 (h * w <= 2^24' in lib.ra_last_error_string()
  tab[1].h, tab[1].w = 3, 50
  rcode = lib.ra_labels_assemble_ragged_i32(one, 3700, tab, one, one, one, 2, 4, 6, 3, rn.RA_LABELS_PLAIN, one, 1 << 30, None, None, None,
                                            None, None, one, None, None, None, None, None)
  assert rcode == rn.RA_E_SHAPE and b'image 1 is 3 x 50, below the network size 4 x 6' in lib.ra_last_error_string()
  assert lib.ra_gt_instance_catalog_ragged_workspace_ints(tab, 2) == 2 * 2 * (2 * 512 + 4)  # two tiles of 1024 pixels at most
