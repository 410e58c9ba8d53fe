"""The image stage on the MI355X: ra_ops.resize_cubic against the NumPy oracle of the recipe (tests/image_oracle.py) and
setup_labels.py from dataset-style folders to the archive.  The recipe is all integer once the tables exist, so every
comparison is array_equal: u8 against the oracle's levels, x against u8.astype(float32) / 255 bit for bit."""
import functools
import os

import numpy as np
import pytest
import torch

import image_oracle as io_
import labels_oracle as lo
import ra_native as rn
import ra_ops as ops

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def case(name):
  """-> (src uint8 [N,Hs,Ws,C], H, W), seeded; the reference of a case is computed once (expected)."""
  rnd = lambda seed, *shape: np.random.RandomState(seed).randint(0, 256, size=shape).astype(np.uint8)
  table = {
      'int_ratio_aligned': lambda: (rnd(1, 1, 16, 32, 3), 4, 8),       # ratio 4, rows of 96 bytes: the staged loads
      'odd_stride_159': lambda: (rnd(2, 1, 37, 53, 3), 16, 24),         # rows of 159 bytes: no 16-byte path
      'enlarge_clamps': lambda: (rnd(3, 1, 9, 7, 3), 20, 13),           # enlarging, taps clamped on all four sides
      'short_source_1x5': lambda: (rnd(4, 1, 1, 5, 3), 3, 4),           # fewer source rows than taps
      'short_source_2x3': lambda: (rnd(5, 1, 2, 3, 3), 5, 2),
      'tiles_batch3': lambda: (rnd(6, 3, 70, 130, 3), 40, 100),         # 10 x 2 tiles, three different images
      'vector_64x128': lambda: (rnd(7, 1, 64, 128, 3), 16, 32),         # Ws * 3 = 384 = 24 x 16: the staged loads, one full tile row
      'one_channel': lambda: (rnd(8, 1, 37, 53, 1), 16, 24),
      'one_channel_vector': lambda: (rnd(9, 2, 32, 64, 1), 12, 20),     # C = 1 with rows of 64 bytes, W % 4 == 0
      'steep_ratio': lambda: (rnd(10, 1, 40, 1600, 3), 2, 66),          # ratio 24 along x: the span of a tile exceeds the staged row
      'element_stores': lambda: (rnd(11, 2, 16, 32, 3), 5, 7),          # staged loads with W * C % 4 != 0
      'checkerboard_17x23': lambda: (io_.checkerboard()[None], 17, 23),
      'checkerboard_40x50': lambda: (io_.checkerboard()[None], 40, 50),
  }
  return table[name]()


@functools.lru_cache(maxsize=None)
def expected(name):
  src, H, W = case(name)
  u8 = io_.resize_cubic_u8(src, H, W)
  u8.setflags(write=False)
  return u8


CASES = ['int_ratio_aligned', 'odd_stride_159', 'enlarge_clamps', 'short_source_1x5', 'short_source_2x3', 'tiles_batch3',
         'vector_64x128', 'one_channel', 'one_channel_vector', 'steep_ratio', 'element_stores', 'checkerboard_17x23',
         'checkerboard_40x50']


def _x_bits(u8):
  return (u8.astype(np.float32) / 255).view(np.uint32)


@pytest.mark.parametrize('name', CASES)
def test_resize_equals_the_oracle(name):
  src, H, W = case(name)
  got = ops.resize_cubic(src, H, W, want=('x', 'u8'))
  u8, x = got['u8'].cpu().numpy(), got['x'].cpu().numpy()
  assert u8.dtype == np.uint8 and x.dtype == np.float32 and u8.shape == x.shape == (src.shape[0], H, W, src.shape[3])
  want = expected(name)
  print('%s: %d of %d levels differ' % (name, int((u8 != want).sum()), want.size))
  assert np.array_equal(u8, want)
  assert np.array_equal(x.view(np.uint32), _x_bits(want))
  if name == 'tiles_batch3':
    assert not np.array_equal(want[0], want[1]) and not np.array_equal(want[1], want[2])
  if name.startswith('checkerboard'):
    assert want.min() == 0 and want.max() == 255


def test_single_outputs_device_input_and_repeat():
  src, H, W = case('tiles_batch3')
  want = expected('tiles_batch3')
  dev = torch.from_numpy(src).cuda()
  only_u8 = ops.resize_cubic(dev, H, W, want=('u8',))
  only_x = ops.resize_cubic(dev, H, W)
  assert set(only_u8) == {'u8'} and set(only_x) == {'x'}
  assert np.array_equal(only_u8['u8'].cpu().numpy(), want)
  bits = only_x['x'].cpu().numpy().view(np.uint32)
  assert np.array_equal(bits, _x_bits(want))
  again = ops.resize_cubic(dev, H, W)['x'].cpu().numpy().view(np.uint32)
  assert np.array_equal(again, bits)
  assert (70, 40, str(dev.device)) in ops._CUBIC_TABLES and (130, 100, str(dev.device)) in ops._CUBIC_TABLES


def test_misaligned_pointers_take_the_narrow_forms():
  """A source that starts 3 bytes into an allocation (no 16-byte loads although Ws * C % 16 == 0) and outputs that start
  off their alignment (element stores although W * C % 4 == 0), through the C ABI."""
  src, H, W = case('vector_64x128')
  want = expected('vector_64x128')
  dev = torch.device('cuda')
  buf = torch.zeros(src.size + 16, dtype=torch.uint8, device=dev)
  buf[3:3 + src.size] = torch.from_numpy(src).reshape(-1).to(dev)
  oy, cy = ops._cubic_tables_dev(64, H, dev)
  ox, cx = ops._cubic_tables_dev(128, W, dev)
  u8 = torch.zeros(want.size + 16, dtype=torch.uint8, device=dev)
  f32 = torch.zeros(want.size + 4, dtype=torch.float32, device=dev)
  rn.check(rn.lib().ra_resize_cubic_u8(buf.data_ptr() + 3, 1, 64, 128, 3, H, W, oy.data_ptr(), cy.data_ptr(), ox.data_ptr(),
                                       cx.data_ptr(), u8.data_ptr() + 1, f32.data_ptr() + 4, rn.stream_ptr()), 'ra_resize_cubic_u8')
  assert np.array_equal(u8[1:1 + want.size].cpu().numpy().reshape(want.shape), want)
  assert np.array_equal(f32[1:1 + want.size].cpu().numpy().view(np.uint32).reshape(want.shape), _x_bits(want))
  assert u8[0].item() == 0 and not u8[1 + want.size:].any().item() and f32[0].item() == 0 and not f32[1 + want.size:].any().item()


def test_argument_checks_launch_nothing():
  dev = torch.device('cuda')
  src = torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device=dev)
  oy, cy = ops._cubic_tables_dev(8, 4, dev)
  out = torch.full((1, 4, 4, 3), 7, dtype=torch.uint8, device=dev)
  call = lambda s, C, H: rn.lib().ra_resize_cubic_u8(s, 1, 8, 8, C, H, 4, oy.data_ptr(), cy.data_ptr(), oy.data_ptr(), cy.data_ptr(),
                                                      out.data_ptr(), None, rn.stream_ptr())
  assert call(src.data_ptr(), 3, 0) == rn.RA_E_SHAPE
  assert call(src.data_ptr(), 2, 4) == rn.RA_E_SHAPE
  assert call(None, 3, 4) == rn.RA_E_SHAPE and b'ra_resize_cubic_u8' in rn.lib().ra_last_error_string()
  torch.cuda.synchronize()
  assert (out == 7).all().item()
  for bad in (src[0], src.float(), src[:, :, :, :2]):
    with pytest.raises(rn.RecAttendError):
      ops.resize_cubic(bad, 4, 4)
  with pytest.raises(rn.RecAttendError):
    ops.resize_cubic(src, 0, 4)


# ---- end to end
def _write(path, data):
  os.makedirs(os.path.dirname(path), exist_ok=True)
  with open(path, 'wb') as f:
    f.write(data)


SIZE = ['--height', '8', '--width', '12', '--timespan', '4']
COLOURS_BGR = np.array([[0, 0, 0], [0, 0, 200], [0, 90, 10], [1, 0, 0]], np.uint8)  # ascending codes: ids 0, 1, 2, 3


def _ids_and_images(seed):
  rng = np.random.RandomState(seed)
  return lo.ellipse_ids(rng, 2, 24, 30, 3), rng.randint(0, 256, size=(2, 24, 30, 3)).astype(np.uint8)


def _existing_stage(ids, dataset, want=('y_gt', 's_gt')):
  got = ops.assemble_labels(ids, 8, 12, 4, dataset, want=want)
  return {k: v.cpu().numpy() for k, v in got.items()}


def test_setup_labels_cvppp_folder(tmp_path):
  import setup_labels as sl
  ids, imgs = _ids_and_images(21)
  assert ids.max() == 3
  folder = str(tmp_path / 'A1')
  for b in range(2):
    _write(os.path.join(folder, 'plant%03d_rgb.png' % (b + 1)), io_.encode_png(imgs[b][:, :, ::-1], 2, filters=[4, 3, 1, 2]))
    _write(os.path.join(folder, 'plant%03d_label.png' % (b + 1)), io_.encode_png(COLOURS_BGR[ids[b]][:, :, ::-1], 2, filters=4))
  out = str(tmp_path / 'out.npz')
  sl.main(['--input', folder, '--images', folder, '--colour_labels', '--dataset', 'cvppp', '--output', out] + SIZE)
  got = dict(np.load(out))
  ref = _existing_stage(ids, 'cvppp')
  assert np.array_equal(got['x'].view(np.uint32), _x_bits(io_.resize_cubic_u8(imgs, 8, 12)))
  assert np.array_equal(got['y_gt'], ref['y_gt']) and np.array_equal(got['s_gt'], ref['s_gt'])
  assert got['orig_size'].tolist() == [[24, 30]] * 2 and got['y_gt'].shape == (2, 4, 8, 12)


def test_setup_labels_cityscapes_pair_and_x_full(tmp_path):
  import ap_oracle as ao
  import setup_labels as sl
  ids, imgs = _ids_and_images(22)
  ids = np.where(ids > 0, 26000 + ids, 0).astype(np.int32)  # cars 26001 ..
  keys = ['aachen/aachen_000001_000019', 'bochum/bochum_000002_000019']
  gt, left = str(tmp_path / 'gtFine'), str(tmp_path / 'leftImg8bit')
  for b, key in enumerate(keys):
    _write(os.path.join(gt, key + '_gtFine_instanceIds.png'), ao.encode_gray16(ids[b].astype(np.uint16), 4))
    _write(os.path.join(left, key + '_leftImg8bit.png'), io_.encode_png(imgs[b][:, :, ::-1], 2, filters=4))
  out = str(tmp_path / 'cs.npz')
  sl.main(['--input', gt, '--images', left, '--dataset', 'cityscapes', '--output', out] + SIZE)
  got = dict(np.load(out))
  ref = _existing_stage(ids, 'cityscapes')
  want_x = _x_bits(io_.resize_cubic_u8(imgs, 8, 12))
  assert np.array_equal(got['x'].view(np.uint32), want_x) and got['orig_size'].tolist() == [[24, 30]] * 2
  assert np.array_equal(got['y_gt'], ref['y_gt']) and np.array_equal(got['s_gt'], ref['s_gt'])
  src = str(tmp_path / 'full.npz')
  np.savez(src, gt_instance_ids=ids, x_full=imgs)
  sl.main(['--input', src, '--dataset', 'cityscapes', '--output', out, '--batch_size', '1'] + SIZE)
  got = dict(np.load(out))
  assert np.array_equal(got['x'].view(np.uint32), want_x) and np.array_equal(got['y_gt'], ref['y_gt'])
  assert got['orig_size'].tolist() == [[24, 30]] * 2
