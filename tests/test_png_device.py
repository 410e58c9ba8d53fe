"""The device PNG encoder's stream format without a device: ra_png_deflate_host (the library's plain sequential C++ form, what
the kernels are compared with in tests/test_png_device_gpu.py) against zlib.decompress and, byte for byte, against the pure-Python
restatement tests/png_deflate_oracle.py; the size bound; every refusal by name; utils/png.wrap read back by the module's own
decoders."""
import ctypes
import zlib

import numpy as np
import pytest

import png_cases as pc
import png_deflate_oracle as ora
import ra_native as rn
import ra_ops as ops
from utils import png


def _raw(img):
  """The scanline bytes zlib.decompress must return: what encode_gray8 / encode_colour8 hand to zlib.compress."""
  img = np.asarray(img)
  rows = (img[:, :, ::-1] if img.ndim == 3 else img).reshape(img.shape[0], -1)
  return np.concatenate([np.zeros((img.shape[0], 1), np.uint8), rows], axis=1).tobytes()


def _check_batch(imgs):
  """imgs: images of one shape.  The host entry's streams against zlib, the Python restatement, the bound and the Adler-32."""
  batch = np.stack(imgs)
  streams, adler = ops.png_deflate_host(batch)
  bpp = 3 if batch.ndim == 4 else 1
  bound = ora.stream_bound(batch.shape[1], batch.shape[2], bpp)
  assert ops.png_deflate_bound(len(imgs), batch.shape[1], batch.shape[2], bpp)[0] == bound
  worst = 0
  for img, z, a in zip(imgs, streams, adler):
    raw = _raw(img)
    assert zlib.decompress(z) == raw
    assert z == ora.stream(img)
    assert int(a) == zlib.adler32(raw) == int.from_bytes(z[-4:], 'big')
    assert len(z) <= bound, (len(z), bound)
    worst = max(worst, len(z) - bound)
  return worst


@pytest.mark.parametrize('case', pc.grid(), ids=lambda c: c[0])
def test_host_stream_against_zlib_and_restatement(case):
  _, kind, W, named = case
  for H in pc.HEIGHTS:
    imgs = [img for name, img in named if name.endswith('-H%d' % H)]
    assert len(imgs) == (5 if kind == 'colour' else 4)
    _check_batch(imgs)


def test_alternating_rows_come_closest_to_the_bound():
  """Every byte but the filter byte a 9-bit literal: a segment takes 3 + 8 + 9 (n - 1) + 10 bits, so the stream stays within 3
  bytes per row of the bound and never goes beyond it."""
  for kind in pc.KINDS:
    for W in pc.WIDTHS:
      img = pc.alternating(kind, 7, W)
      z = ops.png_deflate_host(img[None])[0][0]
      n = 1 + W * (3 if kind == 'colour' else 1)
      assert len(z) == 8 + 7 * (-(-(9 * n + 12) // 8) + 4)
      slack = ora.stream_bound(7, W, 3 if kind == 'colour' else 1) - len(z)
      assert 0 <= slack <= 3 * 7, (kind, W, slack)


@pytest.mark.parametrize('case', pc.run_images(), ids=lambda c: c[0])
def test_every_run_length(case):
  """Stretches of every length 1 .. 300: all 29 length codes, their extra bits, and a 258 match followed by 0 .. 3 bytes."""
  _, kind, img = case
  d = 3 if kind == 'colour' else 1
  rows = (img[:, :, ::-1] if kind == 'colour' else img).reshape(img.shape[0], -1)
  assert pc.expected_stretches(rows, d) >= set(range(1, 301))
  lengths = set()
  for r in ora.scanlines(img)[0]:
    lengths.update(v for k, v in ora.tokens(r, d) if k == 'match')
  assert lengths == set(range(3, 259))  # the restatement's greedy walk emits every match length there is
  _check_batch([img])


def test_white_row_adler_chunk():
  _check_batch([pc.white_row()])


def test_real_width_rows():
  """A row of the flagship width (2048 pixels, 6145 colour bytes): a disc mask row and flat-colour rows."""
  yy, xx = np.mgrid[0:4, 0:2048]
  mask = (((xx - 1000) ** 2 + (yy * 200 - 300) ** 2) < 400 ** 2).astype(np.uint8) * 255
  _check_batch([mask])
  colour = np.zeros((4, 2048, 3), np.uint8)
  colour[mask > 0] = (43, 57, 192)
  colour[:, 1500:1700] = (18, 156, 243)
  _check_batch([colour])


def test_float_source_and_plane_list():
  """float32 planes quantised in the load as (y * 255).to(uint8), picked by a list that skips, repeats and reorders."""
  ks = np.arange(256, dtype=np.float32) / np.float32(255.0)
  y = np.zeros((5, 6, 70), np.float32)
  y[0] = 1.0
  y[1] = 0.5
  y[2] = np.resize(ks, (6, 70))
  y[3] = 0.999
  y[4] = np.random.RandomState(3).rand(6, 70) > 0.5
  want = (y * np.float32(255.0)).astype(np.uint8)
  assert want[1, 0, 0] == 127 and want[3, 0, 0] == 254 and want[0, 0, 0] == 255
  planes = [4, 0, 0, 3, 1]  # skips 2, repeats 0, out of order
  streams, _ = ops.png_deflate_host(y, planes)
  assert len(streams) == len(planes)
  for p, z in zip(planes, streams):
    assert zlib.decompress(z) == _raw(want[p])
    assert z == ora.stream(want[p])
  full, _ = ops.png_deflate_host(y)
  assert [zlib.decompress(z) for z in full] == [_raw(w) for w in want]


def test_wrap_is_read_back():
  """Files from wrap() decode with the module's own readers, decode_gray8 (filter 0 only) included."""
  grey = np.random.RandomState(5).randint(0, 3, size=(9, 33)).astype(np.uint8) * 100
  colour = np.random.RandomState(6).randint(0, 2, size=(9, 33, 3)).astype(np.uint8) * 255
  zg = ops.png_deflate_host(grey[None])[0][0]
  zc = ops.png_deflate_host(colour[None])[0][0]
  assert np.array_equal(png.decode_gray8(png.wrap(9, 33, 0, zg)), grey)
  assert np.array_equal(png.decode_colour8(png.wrap(9, 33, 2, zc)), colour)
  assert np.array_equal(png.decode_colour8(png.wrap(9, 33, 0, zg)), np.repeat(grey[:, :, None], 3, axis=2))
  with pytest.raises(ValueError):
    png.wrap(9, 33, 6, zc)


# ---- refusals: the code by name, the message naming the argument, the outputs untouched
def _call(fn, src, kind, M, N, H, W, out_bytes=None, plane=None, null=(), ws=None, ws_bytes=0):
  bpp = 3 if kind == rn.RA_PNG_BGR8 else 1
  cap = 8 + max(1, H) * (-(-9 * (1 + max(1, W) * bpp) // 8) + 7)
  out = np.full((max(1, N) * min(cap, 1 << 16),), 0xAB, np.uint8)
  sizes, offsets, adler = np.full((8,), -7, np.int32), np.full((8,), 77, np.uint64), np.full((8,), 99, np.uint32)
  args = {'src': rn.ptr(src), 'out': rn.ptr(out), 'sizes': rn.ptr(sizes), 'offsets': rn.ptr(offsets), 'adler': rn.ptr(adler)}
  for k in null:
    args[k] = None
  tail = (ws, ws_bytes) if fn == 'ra_png_deflate_host' else (ws, ws_bytes, None)
  rc = getattr(rn.lib(), fn)(args['src'], kind, M, N, H, W, rn.ptr(plane), args['out'], out.size if out_bytes is None else out_bytes,
                             args['sizes'], args['offsets'], args['adler'], *tail)
  assert (out == 0xAB).all() and (sizes == -7).all() and (offsets == 77).all() and (adler == 99).all()
  return rc, (rn.lib().ra_last_error_string() or b'').decode()


REFUSALS = [
    # (what, kind, M, N, H, W, keyword arguments, the code, a word of the message)
    ('N = 0', 0, 1, 0, 2, 4, {}, 'RA_E_SHAPE', 'N='),
    ('N above the cap', 0, 1, 65536, 2, 4, {'plane': np.zeros(8, np.int32)}, 'RA_E_SHAPE', 'N='),
    ('M = 0', 0, 0, 1, 2, 4, {}, 'RA_E_SHAPE', 'M='),
    ('H = 0', 0, 1, 1, 0, 4, {}, 'RA_E_SHAPE', 'H='),
    ('W = 0', 0, 1, 1, 2, 0, {}, 'RA_E_SHAPE', 'W='),
    ('N > M without a list', 0, 1, 2, 2, 4, {}, 'RA_E_SHAPE', 'plane list'),
    ('row too long, grey', 0, 1, 1, 1, 24576, {}, 'RA_E_SHAPE', 'scanlines'),
    ('row too long, colour', 1, 1, 1, 1, 8192, {}, 'RA_E_SHAPE', 'scanlines'),
    ('stream bound of 2^31', 0, 1, 1, 90000, 24575, {}, 'RA_E_SHAPE', '2^31'),
    ('float image of 2^31 bytes', 2, 1, 1, 32768, 16384, {}, 'RA_E_SHAPE', '2^31'),
    ('another kind', 3, 1, 1, 2, 4, {}, 'RA_E_INVALID', 'kind'),
    ('NULL src', 0, 1, 1, 2, 4, {'null': ('src',)}, 'RA_E_INVALID', 'NULL'),
    ('NULL out', 0, 1, 1, 2, 4, {'null': ('out',)}, 'RA_E_INVALID', 'NULL'),
    ('NULL sizes', 0, 1, 1, 2, 4, {'null': ('sizes',)}, 'RA_E_INVALID', 'NULL'),
    ('NULL offsets', 0, 1, 1, 2, 4, {'null': ('offsets',)}, 'RA_E_INVALID', 'NULL'),
    ('NULL adler', 0, 1, 1, 2, 4, {'null': ('adler',)}, 'RA_E_INVALID', 'NULL'),
    ('capacity one byte short', 0, 1, 1, 2, 4, {'out_bytes': 8 + 2 * 13 - 1}, 'RA_E_WORKSPACE', 'out_bytes'),
]


@pytest.mark.parametrize('fn', ['ra_png_deflate_host', 'ra_png_deflate_u8'])
@pytest.mark.parametrize('case', REFUSALS, ids=lambda c: c[0])
def test_refusals_by_name(fn, case):
  """Both entries refuse on the host before anything is read, written or launched: the device entry is called here with host
  pointers and no device, and must return before it would touch either."""
  what, kind, M, N, H, W, kw, code, word = case
  src = np.zeros((64,), np.uint8)
  rc, msg = _call(fn, src, kind, M, N, H, W, **kw)
  assert rc == getattr(rn, code), (what, rc, msg)
  assert fn in msg and word in msg, msg


def test_device_entry_refuses_a_bad_workspace_before_any_launch():
  src = np.zeros((64,), np.uint8)
  ws = np.zeros((4096,), np.uint8)
  need = ops.png_deflate_bound(1, 2, 4, 1)[1]
  base = rn.ptr(ws) + (-rn.ptr(ws) % 16)
  for what, p, nbytes in (('NULL', None, need), ('short', base, need - 1), ('not aligned', base + 8, need)):
    rc, msg = _call('ra_png_deflate_u8', src, 0, 1, 1, 2, 4, ws=p, ws_bytes=nbytes)
    assert rc == rn.RA_E_WORKSPACE and 'ws' in msg, (what, rc, msg)


def test_host_entry_refuses_a_plane_index_outside_the_source():
  src = np.zeros((2, 2, 4), np.uint8)
  for bad in (-1, 2):
    rc, msg = _call('ra_png_deflate_host', src, 0, 2, 2, 2, 4, plane=np.array([0, bad], np.int32))
    assert rc == rn.RA_E_SHAPE and 'plane[1]' in msg, (rc, msg)


def test_bound_query():
  lib = rn.lib()
  a, b = ctypes.c_ulonglong(5), ctypes.c_ulonglong(6)
  for args, word in (((1, 2, 4, 2), 'bpp'), ((0, 2, 4, 1), 'N='), ((1, 0, 4, 1), 'H='), ((1, 2, 0, 1), 'W='),
                     ((1, 1, 8192, 3), 'scanlines'), ((1, 90000, 24575, 1), '2^31')):
    assert lib.ra_png_deflate_bound(*args, ctypes.addressof(a), ctypes.addressof(b)) == rn.RA_E_SHAPE
    assert word in lib.ra_last_error_string().decode()
    assert (a.value, b.value) == (5, 6)
  assert lib.ra_png_deflate_bound(1, 2, 4, 1, None, ctypes.addressof(b)) == rn.RA_E_INVALID
  for N, H, W, bpp in ((1, 1, 1, 1), (20, 1024, 2048, 1), (1, 1024, 2048, 3), (3, 7, 1031, 3)):
    stream, ws = ops.png_deflate_bound(N, H, W, bpp)
    n = 1 + W * bpp
    assert stream == 8 + H * (-(-9 * n // 8) + 7) == ora.stream_bound(H, W, bpp)
    assert ws >= N * H * (16 + ora.segment_bound(n))  # a record and a worst-case slot per segment


def test_module_imports_without_the_library(monkeypatch):
  """utils/png's host functions need neither the library nor ra_ops: only the _dev functions import them, when called."""
  import importlib
  import sys
  monkeypatch.setitem(sys.modules, 'ra_ops', None)
  monkeypatch.setitem(sys.modules, 'ra_native', None)
  mod = importlib.reload(png)
  try:
    img = np.arange(12, dtype=np.uint8).reshape(3, 4)
    assert np.array_equal(mod.decode_gray8(mod.encode_gray8(img)), img)
    assert np.array_equal(mod.decode_gray8(mod.wrap(3, 4, 0, zlib.compress(_raw(img)))), img)
    with pytest.raises(ImportError):
      mod.encode_gray8_dev(None)
  finally:
    monkeypatch.undo()
    importlib.reload(png)
