"""The image stage without a device: the NumPy oracle (tests/image_oracle.py) against an independent bicubic and against
properties that need no oracle, the library's host entry points (tables, PNG unfilter) against the oracle and the NumPy
unfilter, utils/png.py's colour reader, and setup_labels.py's --images / --colour_labels with the device op replaced by the
oracle."""
import ctypes
import os

import numpy as np
import pytest

import image_oracle as io_
import ra_native as rn

ALL_SHAPES = io_.SHAPES + [io_.KITTI_SHAPE]


def _random_u8(seed, *shape):
  return np.random.RandomState(seed).randint(0, 256, size=shape).astype(np.uint8)


# ---- the oracle against an independent implementation
def test_oracle_against_float64_bicubic():
  """torch's bicubic (A = -0.75, align_corners=False: the same sample positions and clamped taps) in float64, unrounded,
  clipped to [0, 255], against the recipe's uint8.  The recipe rounds the weights to 11 bits and the result to a level:
  at most 1.0 grey level apart (observed: profiles/image_stage.txt)."""
  import torch
  import torch.nn.functional as F
  worst = 0.0
  for k, ((Hs, Ws), (H, W)) in enumerate(ALL_SHAPES):
    img = _random_u8(100 + k, Hs, Ws, 3)
    got = io_.resize_cubic_u8(img, H, W)
    t = torch.from_numpy(img.astype(np.float64)).permute(2, 0, 1)[None]
    ref = F.interpolate(t, size=(H, W), mode='bicubic', align_corners=False)[0].permute(1, 2, 0).numpy().clip(0, 255)
    diff = float(np.abs(got.astype(np.float64) - ref).max())
    print('oracle vs float64 bicubic, %d x %d -> %d x %d: max |diff| = %.4f grey levels' % (Hs, Ws, H, W, diff))
    worst = max(worst, diff)
    assert diff <= 1.0, ((Hs, Ws), (H, W), diff)
  print('oracle vs float64 bicubic, all shapes: max |diff| = %.4f' % worst)


# ---- properties that need no oracle
def test_identity():
  img = _random_u8(1, 8, 8, 3)
  assert np.array_equal(io_.resize_cubic_u8(img, 8, 8), img)
  ofs, coef = io_.cubic_table(8, 8)
  assert ofs.tolist() == list(range(8)) and (coef == np.array([0, 2048, 0, 0], np.int16)).all()


@pytest.mark.parametrize('value', [1, 127, 200, 255])
def test_constant_stays_constant(value):
  """A weight sum of 2048 + e, e in {-1, 0, 1}, on each axis gives v = value * (2048 + ey) * (2048 + ex); the excess over
  value << 22 is below value * 4100 < 2^21, so the rounding shift returns value."""
  for (Hs, Ws), (H, W) in ALL_SHAPES:
    got = io_.resize_cubic_u8(np.full((Hs, Ws, 3), value, np.uint8), H, W)
    assert (got == value).all(), ((Hs, Ws), (H, W))


@pytest.mark.parametrize('size', [(17, 23), (40, 50)])
def test_checkerboard_meets_both_clamps(size):
  board = io_.checkerboard()
  v = io_.resize_cubic_unclipped(board, *size) / float(1 << 22)
  assert (v < 0).mean() > 0.2 and (v > 255).mean() > 0.2
  got = io_.resize_cubic_u8(board, *size)
  assert got.min() == 0 and got.max() == 255


# ---- the library's tables
def _lib_tables(S, D):
  ofs, coef = np.full((D,), -12345, np.int32), np.full((D, 4), -12345, np.int16)
  assert rn.lib().ra_resize_cubic_tables(S, D, ofs.ctypes.data, coef.ctypes.data) == 0
  return ofs, coef


def test_tables_equal_the_oracle():
  pairs = [(S, D) for S in range(1, 65) for D in range(1, 65)]
  pairs += [(2048, 512), (1024, 256), (1242, 448), (375, 128), (530, 224), (500, 224)]
  sums = set()
  for S, D in pairs:
    ofs, coef = _lib_tables(S, D)
    want_ofs, want_coef = io_.cubic_table(S, D)
    assert np.array_equal(ofs, want_ofs) and np.array_equal(coef, want_coef), (S, D)
    sums |= set(coef.astype(np.int32).sum(axis=1).tolist())
  assert sums <= {2047, 2048, 2049}, sums


def test_tables_through_ra_ops_and_argument_checks():
  import ra_ops as ops
  ofs, coef = ops.cubic_tables(1242, 448)
  want = io_.cubic_table(1242, 448)
  assert ofs.dtype == np.int32 and coef.dtype == np.int16 and coef.shape == (448, 4)
  assert np.array_equal(ofs, want[0]) and np.array_equal(coef, want[1])
  lib = rn.lib()
  one = np.zeros(64, np.int32).ctypes.data
  assert lib.ra_resize_cubic_tables(0, 4, one, one) == rn.RA_E_SHAPE and lib.ra_resize_cubic_tables(4, 0, one, one) == rn.RA_E_SHAPE
  assert lib.ra_resize_cubic_tables(4, 4, None, one) == rn.RA_E_SHAPE and b'ra_resize_cubic_tables' in lib.ra_last_error_string()
  with pytest.raises(rn.RecAttendError, match='ra_resize_cubic_tables'):
    ops.cubic_tables(0, 3)


def test_resize_argument_checks_without_gpu():
  """Refused before anything is read or launched: any non-null address will do."""
  lib = rn.lib()
  one = 16
  call = lambda src=one, N=1, Hs=8, Ws=8, C=3, H=4, W=4, u8=one, f32=one: lib.ra_resize_cubic_u8(
      src, N, Hs, Ws, C, H, W, one, one, one, one, u8, f32, None)
  for kw in (dict(H=0), dict(W=0), dict(Hs=0), dict(C=2), dict(C=4), dict(src=None), dict(N=0), dict(N=65536),
             dict(Hs=1 << 15, Ws=1 << 15), dict(H=1 << 14, W=1 << 14), dict(H=1 << 15, W=1 << 15, f32=None)):
    assert call(**kw) == rn.RA_E_SHAPE and b'ra_resize_cubic_u8' in lib.ra_last_error_string(), kw
  assert lib.ra_resize_cubic_u8(one, 1, 8, 8, 3, 4, 4, None, one, one, one, one, one, None) == rn.RA_E_SHAPE


def test_no_device_raises(monkeypatch):
  import torch
  import ra_ops as ops
  monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
  with pytest.raises(rn.RecAttendError, match='no CPU fallback'):
    ops.resize_cubic(np.zeros((1, 8, 8, 3), np.uint8), 4, 4)
  with pytest.raises(rn.RecAttendError, match='no CPU fallback'):
    ops.resize_cubic(torch.zeros((1, 8, 8, 3), dtype=torch.uint8), 4, 4)
  with pytest.raises(rn.RecAttendError, match='uint8'):
    ops.resize_cubic(np.zeros((1, 8, 8, 3), np.float32), 4, 4)
  with pytest.raises(rn.RecAttendError, match='want'):
    ops.resize_cubic(np.zeros((1, 8, 8, 3), np.uint8), 4, 4, want=('y',))


# ---- the compiled unfilter
def _scanlines(rng, H, stride, filters):
  raw = rng.randint(0, 256, size=(H, stride + 1)).astype(np.uint8)
  raw[:, 0] = [filters[r % len(filters)] for r in range(H)]
  return raw


def _lib_unfilter(raw, H, stride, bpp):
  out = np.full((H, stride), 0xA5, np.uint8)
  rc = rn.lib().ra_png_unfilter_u8(np.ascontiguousarray(raw).ctypes.data, H, stride, bpp, out.ctypes.data)
  return rc, out


def test_unfilter_equals_the_numpy_one():
  from utils import png
  rng = np.random.RandomState(7)
  orders = [[4, 3, 2, 1, 0], [3, 4, 0, 1, 2], [0, 1, 2, 3, 4], [1], [2], [3], [4]]  # Paeth and Average on row 0 among them
  for bpp in (1, 2, 3, 4, 6):
    for width in (1, 2, 5, 33):
      for H in (1, 7):
        for filters in orders:
          stride = width * bpp
          raw = _scanlines(rng, H, stride, filters)
          rc, got = _lib_unfilter(raw, H, stride, bpp)
          assert rc == 0
          assert np.array_equal(got, png._unfilter_diagonals(raw, H, stride, bpp)), (bpp, width, H, filters)


def test_unfilter_refuses_filter_type_5_and_bad_sizes():
  raw = _scanlines(np.random.RandomState(0), 3, 6, [0, 5, 1])
  rc, _ = _lib_unfilter(raw, 3, 6, 3)
  assert rc == rn.RA_E_SHAPE and b'row 1 has filter type 5' in rn.lib().ra_last_error_string()
  out = np.zeros(64, np.uint8)
  for H, stride, bpp in ((0, 6, 3), (3, 0, 3), (3, 6, 0), (3, 6, 9), (3, 7, 3), (-1, 6, 3)):  # refused before anything is read
    assert rn.lib().ra_png_unfilter_u8(raw.ctypes.data, H, stride, bpp, out.ctypes.data) == rn.RA_E_SHAPE, (H, stride, bpp)
  assert rn.lib().ra_png_unfilter_u8(None, 3, 6, 3, raw.ctypes.data) == rn.RA_E_SHAPE


def test_unfilter_is_used_and_falls_back(monkeypatch):
  """_unfilter takes the compiled loop for Average / Paeth rows when the library loads, the NumPy diagonals when it does
  not, and gives the same bytes either way."""
  from utils import png
  raw = _scanlines(np.random.RandomState(3), 5, 12, [4, 3, 1, 2, 0])
  calls = []
  native = png._unfilter_native
  monkeypatch.setattr(png, '_unfilter_native', lambda *a: calls.append('native') or native(*a))
  a = png._unfilter(raw.tobytes(), 5, 12, 3)
  assert calls == ['native']
  monkeypatch.setattr(png, '_NATIVE', [None])
  b = png._unfilter(raw.tobytes(), 5, 12, 3)
  assert calls == ['native'] and np.array_equal(a, b) and np.array_equal(a, png._unfilter_diagonals(raw, 5, 12, 3))
  monkeypatch.setattr(png, '_NATIVE', [])
  monkeypatch.setattr(rn, 'LIB_PATH', os.path.join(os.path.dirname(rn.LIB_PATH), 'nope.so'))
  monkeypatch.setattr(rn, '_lib', None)
  assert np.array_equal(png._unfilter(raw.tobytes(), 5, 12, 3), a) and png._NATIVE == [None]


# ---- colour PNG files
def _rgb(seed=5, H=7, W=9):
  img = _random_u8(seed, H, W, 3)
  img[..., 0] |= 0x80  # the three channels differ: R high, B low
  img[..., 2] &= 0x7f
  return img


@pytest.mark.parametrize('filters', [0, 1, 2, 3, 4, [4, 0, 3, 1, 2]])
def test_decode_rgb(filters):
  from utils import png
  img = _rgb()
  got = png.decode_colour8(io_.encode_png(img, 2, filters=filters, idat_split=3))
  assert got.dtype == np.uint8 and got.shape == (7, 9, 3) and got.flags['C_CONTIGUOUS']
  assert np.array_equal(got, img[:, :, ::-1]) and not np.array_equal(got, img)  # BGR


def test_decode_rgba_grey_and_read(tmp_path):
  from utils import png
  img = _rgb(6)
  for alpha in (0, 255, None):
    a = _random_u8(9, 7, 9, 1) if alpha is None else np.full((7, 9, 1), alpha, np.uint8)
    got = png.decode_colour8(io_.encode_png(np.concatenate([img, a], axis=2), 6, filters=[4, 3]))
    assert np.array_equal(got, img[:, :, ::-1])
  grey = _random_u8(8, 5, 6)
  got = png.decode_colour8(io_.encode_png(grey, 0, filters=[1, 4]))
  assert got.shape == (5, 6, 3) and all(np.array_equal(got[..., c], grey) for c in range(3))
  path = str(tmp_path / 'a.png')
  with open(path, 'wb') as f:
    f.write(io_.encode_png(img, 2, filters=4))
  assert np.array_equal(png.read_colour8(path), img[:, :, ::-1])


@pytest.mark.parametrize('depth', [1, 2, 4, 8])
def test_decode_palette(depth):
  from utils import png
  rng = np.random.RandomState(depth)
  n = 1 << depth
  palette = rng.randint(0, 256, size=(n, 3)).astype(np.uint8)
  W = 13  # no multiple of 8, 4 or 2 pixels per byte
  idx = rng.randint(0, n, size=(6, W)).astype(np.uint8)
  tRNS = io_._chunk(b'tRNS', bytes(n))
  data = io_.encode_png(idx, 3, depth=depth, filters=[0, 2, 1, 4, 3], palette=palette)
  cut = data.index(b'IDAT') - 4
  for blob in (data, data[:cut] + tRNS + data[cut:]):  # tRNS is ignored
    assert np.array_equal(png.decode_colour8(blob), palette[idx][:, :, ::-1])
  if depth > 1:
    with pytest.raises(ValueError, match='palette index'):
      png.decode_colour8(io_.encode_png(idx | (n - 1), 3, depth=depth, palette=palette[:n - 1]))


def test_decode_refusals():
  from utils import png
  img = _rgb()
  good = io_.encode_png(img, 2, filters=4)
  with pytest.raises(ValueError, match='bit depth 8, colour type 2, interlace 1'):
    png.decode_colour8(io_.encode_png(img, 2, interlace=1))
  with pytest.raises(ValueError, match='bit depth 16, colour type 2, interlace 0'):
    png.decode_colour8(io_.encode_png(img.astype(np.uint16) * 257, 2, depth=16))
  with pytest.raises(ValueError, match='bit depth 16, colour type 0'):
    png.decode_colour8(io_.encode_png(img[..., 0].astype(np.uint16), 0, depth=16))
  bad = bytearray(good)
  bad[good.index(b'IDAT') + 6] ^= 0x10
  with pytest.raises(ValueError, match='bad CRC'):
    png.decode_colour8(bytes(bad))
  for cut in (len(good) - 5, good.index(b'IDAT') + 10, 20):
    with pytest.raises(ValueError):
      png.decode_colour8(good[:cut])
  with pytest.raises(ValueError):  # whole chunks, but no image data after the header
    png.decode_colour8(good[:good.index(b'IDAT') - 4] + io_._chunk(b'IEND', b''))
  with pytest.raises(ValueError, match='PLTE'):
    png.decode_colour8(io_.encode_png(img[..., 0] & 3, 3, depth=2))
  with pytest.raises(ValueError, match='not a PNG'):
    png.decode_colour8(b'JFIF' + good)


def test_decode_files_written_by_pil(tmp_path):
  Image = pytest.importorskip('PIL.Image')
  from utils import png
  img = _random_u8(11, 37, 53, 3)
  path = str(tmp_path / 'rgb.png')
  Image.fromarray(img).save(path)
  assert np.array_equal(png.read_colour8(path), np.asarray(Image.open(path).convert('RGB'))[:, :, ::-1])
  pal = Image.fromarray(img).quantize(17)
  path = str(tmp_path / 'pal.png')
  pal.save(path)
  assert np.array_equal(png.read_colour8(path), np.asarray(Image.open(path).convert('RGB'))[:, :, ::-1])


# ---- the command line
def _fake_ops(monkeypatch):
  """The device ops replaced by their oracles, as tests/test_labels.py does for the label stage."""
  import torch
  import labels_oracle as lo
  import ra_ops as ops
  calls = []

  def fake_labels(gt_ids, H, W, T, ds, want=(), names=None):
    ref = lo.assemble(gt_ids, H, W, T, lo.CITYSCAPES if ds == 'cityscapes' else lo.PLAIN)
    return {k: torch.from_numpy(np.ascontiguousarray(ref[k])) for k in want}

  def fake_resize(src, H, W, want=('x',)):
    calls.append(tuple(src.shape))
    u8 = io_.resize_cubic_u8(src, H, W)
    return {k: torch.from_numpy({'x': io_.to_x(u8), 'u8': u8}[k]) for k in want}

  monkeypatch.setattr(ops, 'assemble_labels', fake_labels)
  monkeypatch.setattr(ops, 'resize_cubic', fake_resize)
  monkeypatch.setattr(torch.cuda, 'is_available', lambda: True)
  return calls


def _write(path, data):
  os.makedirs(os.path.dirname(path), exist_ok=True)
  with open(path, 'wb') as f:
    f.write(data)


def _id_images(n=2, Hf=24, Wf=30):
  """int32 [n,Hf,Wf]: three rectangles of ids 1, 2, 3 of different areas on a background of 0."""
  ids = np.zeros((n, Hf, Wf), np.int32)
  for b in range(n):
    ids[b, 2:10, 3 + b:12] = 1
    ids[b, 12:22, 5:25 - b] = 2
    ids[b, 3:9, 18:28] = 3
  return ids


COLOURS_BGR = np.array([[0, 0, 0], [0, 0, 200], [0, 90, 10], [1, 0, 0]], np.uint8)  # codes 0 < 200 < 23050 < 65536: ids 0, 1, 2, 3
SIZE = ['--height', '8', '--width', '12', '--timespan', '4']


def test_command_line_cvppp(tmp_path, monkeypatch):
  import labels_oracle as lo
  import setup_labels as sl
  calls = _fake_ops(monkeypatch)
  ids = _id_images()
  imgs = _random_u8(2, 2, 24, 30, 3)  # BGR, as the archive must hold them
  folder = str(tmp_path / 'A1')
  for b in range(2):
    _write(os.path.join(folder, 'plant%03d_rgb.png' % (b + 1)), io_.encode_png(imgs[b][:, :, ::-1], 2, filters=[4, 3, 1]))
    _write(os.path.join(folder, 'plant%03d_label.png' % (b + 1)), io_.encode_png(COLOURS_BGR[ids[b]][:, :, ::-1], 2, filters=4))
    _write(os.path.join(folder, 'plant%03d_fg.png' % (b + 1)), io_.encode_png((ids[b] > 0).astype(np.uint8), 0))
  out = str(tmp_path / 'out.npz')
  sl.main(['--input', folder, '--images', folder, '--colour_labels', '--dataset', 'cvppp', '--output', out, '--batch_size', '1'] + SIZE)
  got = dict(np.load(out))
  ref = lo.assemble(ids, 8, 12, 4, lo.PLAIN)
  assert set(got) == {'x', 'y_gt', 's_gt', 'orig_size'} and calls == [(1, 24, 30, 3)] * 2
  assert got['x'].dtype == np.float32 and np.array_equal(got['x'], io_.to_x(io_.resize_cubic_u8(imgs, 8, 12)))
  assert np.array_equal(got['y_gt'], ref['y_gt']) and np.array_equal(got['s_gt'], ref['s_gt'])
  assert got['orig_size'].dtype == np.int32 and got['orig_size'].tolist() == [[24, 30]] * 2
  # a missing image and a size mismatch are named; without --colour_labels the colour label file is refused as before
  with pytest.raises(rn.RecAttendError, match='colour type 2'):
    sl.main(['--input', folder, '--images', folder, '--dataset', 'cvppp', '--output', out] + SIZE)
  with pytest.raises(rn.RecAttendError, match='colour type 2'):
    sl.main(['--input', folder, '--dataset', 'cvppp', '--output', out] + SIZE)
  _write(os.path.join(folder, 'plant002_rgb.png'), io_.encode_png(imgs[1][:20, :, ::-1], 2))
  with pytest.raises(rn.RecAttendError, match=r'plant002_rgb\.png is 20 x 30.*plant002_label\.png 24 x 30'):
    sl.main(['--input', folder, '--images', folder, '--colour_labels', '--dataset', 'cvppp', '--output', out] + SIZE)
  os.remove(os.path.join(folder, 'plant002_rgb.png'))
  with pytest.raises(rn.RecAttendError, match=r'plant002_label\.png: no image plant002_rgb\.png'):
    sl.main(['--input', folder, '--images', folder, '--colour_labels', '--dataset', 'cvppp', '--output', out] + SIZE)


def test_command_line_cityscapes_and_kitti(tmp_path, monkeypatch):
  import ap_oracle as ao
  import labels_oracle as lo
  import setup_labels as sl
  _fake_ops(monkeypatch)
  ids = _id_images() * 1000 + 24000 * (_id_images() > 0)  # persons 25000, 26000, 27000 -> ids of three labels
  imgs = _random_u8(3, 2, 24, 30, 3)
  keys = ['aachen/aachen_000001_000019', 'bochum/bochum_000002_000019']
  gt, left = str(tmp_path / 'gtFine' / 'train'), str(tmp_path / 'leftImg8bit')
  for b, key in enumerate(keys):
    _write(os.path.join(gt, key + '_gtFine_instanceIds.png'), ao.encode_gray16(ids[b].astype(np.uint16), 4))
    _write(os.path.join(gt, key + '_gtFine_labelIds.png'), io_.encode_png((ids[b] // 1000).astype(np.uint8), 0))  # filtered out
    _write(os.path.join(left, 'train', key + '_leftImg8bit.png'), io_.encode_png(imgs[b][:, :, ::-1], 2, filters=4))
  out = str(tmp_path / 'cs.npz')
  sl.main(['--input', gt, '--images', left, '--dataset', 'cityscapes', '--target', 'fg_model', '--output', out] + SIZE)
  got = dict(np.load(out))
  ref = lo.assemble(ids, 8, 12, 4, lo.CITYSCAPES)
  assert set(got) == {'x', 'y_gt', 'd_gt', 'fg_gt_full', 'names', 'orig_size'}
  assert got['names'].tolist() == [os.path.basename(k) + '_gtFine_instanceIds.png' for k in keys]
  assert np.array_equal(got['x'], io_.to_x(io_.resize_cubic_u8(imgs, 8, 12))) and np.array_equal(got['y_gt'], ref['c_gt'])
  # KITTI: gt/ and images/ hold the same names; colour labels
  small = _id_images()
  kgt, kim = str(tmp_path / 'kitti' / 'gt'), str(tmp_path / 'kitti' / 'images')
  for b in range(2):
    _write(os.path.join(kgt, '%06d.png' % b), io_.encode_png(COLOURS_BGR[small[b]][:, :, ::-1], 2, filters=1))
    _write(os.path.join(kim, '%06d.png' % b), io_.encode_png(imgs[b][:, :, ::-1], 2, filters=2))
  sl.main(['--input', kgt, '--images', kim, '--colour_labels', '--dataset', 'kitti', '--output', out] + SIZE)
  got = dict(np.load(out))
  assert np.array_equal(got['x'], io_.to_x(io_.resize_cubic_u8(imgs, 8, 12)))
  assert np.array_equal(got['y_gt'], lo.assemble(small, 8, 12, 4, lo.PLAIN)['y_gt'])
  os.remove(os.path.join(kim, '000001.png'))
  with pytest.raises(rn.RecAttendError, match=r'000001\.png: no image 000001\.png'):
    sl.main(['--input', kgt, '--images', kim, '--colour_labels', '--dataset', 'kitti', '--output', out] + SIZE)
  with pytest.raises(rn.RecAttendError, match='folders'):
    sl.main(['--input', kgt, '--images', str(tmp_path / 'nowhere'), '--dataset', 'kitti', '--output', out] + SIZE)


def test_colour_labels_to_ids(tmp_path):
  import ra_ops as ops
  import setup_labels as sl
  lab = _id_images(1)[0]
  bgr = COLOURS_BGR[lab]
  assert np.array_equal(sl.colour_ids(bgr, 'a.png'), lab)
  # two colours that differ in the blue byte alone, the most significant of the code: (B, G, R) = (1, 0, 5) > (0, 255, 255)
  two = np.array([[0, 0, 0], [1, 0, 5], [0, 255, 255]], np.uint8)
  assert np.array_equal(sl.colour_ids(two[np.array([[0, 1, 2, 1]])], 'b.png'), [[0, 2, 1, 2]])
  blue = np.array([[0, 7, 9], [3, 7, 9], [2, 7, 9]], np.uint8)  # no background at all: ids from 1
  assert np.array_equal(sl.colour_ids(blue[np.array([[0, 1, 2]])], 'c.png'), [[1, 3, 2]])
  # MAX_GT - 1 colours beside the background pass, 256 are refused by name
  many = np.zeros((1, ops.MAX_GT + 1, 3), np.uint8)
  many[0, :, 1] = np.arange(ops.MAX_GT + 1) % 256
  many[0, :, 0] = np.arange(ops.MAX_GT + 1) // 256
  assert sl.colour_ids(many[:, :ops.MAX_GT], 'd.png').max() == ops.MAX_GT - 1
  with pytest.raises(rn.RecAttendError, match=r'many\.png: 256 distinct colours'):
    sl.colour_ids(many, 'many.png')
  # through the reader: a colour file under the flag, a grey file unchanged, a broken file named
  path = str(tmp_path / 'lab.png')
  _write(path, io_.encode_png(bgr[:, :, ::-1], 2, filters=3))
  assert np.array_equal(sl.read_label_png(path, colour_labels=True), lab)
  grey = str(tmp_path / 'grey.png')
  _write(grey, io_.encode_png(lab.astype(np.uint8) * 50, 0))
  assert np.array_equal(sl.read_label_png(grey, colour_labels=True), lab * 50)
  with pytest.raises(rn.RecAttendError, match='colour type 2'):
    sl.read_label_png(path)
  _write(path, io_.encode_png(bgr[:, :, ::-1], 2, interlace=1))
  with pytest.raises(rn.RecAttendError, match=r'lab\.png.*interlace 1'):
    sl.read_label_png(path, colour_labels=True)


def test_command_line_x_full(tmp_path, monkeypatch):
  import setup_labels as sl
  calls = _fake_ops(monkeypatch)
  ids, imgs = _id_images(3), _random_u8(4, 3, 24, 30, 3)
  src, out = str(tmp_path / 'in.npz'), str(tmp_path / 'out.npz')
  np.savez(src, gt_instance_ids=ids, x_full=imgs)
  sl.main(['--input', src, '--dataset', 'kitti', '--output', out, '--batch_size', '2'] + SIZE)
  got = dict(np.load(out))
  assert calls == [(2, 24, 30, 3), (1, 24, 30, 3)] and got['orig_size'].tolist() == [[24, 30]] * 3
  assert np.array_equal(got['x'], io_.to_x(io_.resize_cubic_u8(imgs, 8, 12)))
  np.savez(src, gt_instance_ids=ids, x_full=imgs[:, :20])
  with pytest.raises(rn.RecAttendError, match='x_full'):
    sl.main(['--input', src, '--dataset', 'kitti', '--output', out] + SIZE)
  x = np.zeros((3, 8, 12, 3), np.float32)
  np.savez(src, gt_instance_ids=ids, x_full=imgs, x=x)  # an x at network size wins, as before
  sl.main(['--input', src, '--dataset', 'kitti', '--output', out] + SIZE)
  assert 'orig_size' not in np.load(out) and not np.load(out)['x'].any()
