"""The device PNG encoder's "dynamic" stream format without a device: ra_png_deflate_dyn_host (the library's sequential C++ form,
what the kernels are compared with in tests/test_png_dynamic_gpu.py) against zlib.decompress and, byte for byte, against the
pure-Python restatement tests/png_dynamic_oracle.py; the limiter alone (ra_png_huffman_lengths) on histograms that need it; the
size bound; that the case grid reaches every bit alignment the placement kernel has to handle; the refusals by name; the keywords
and the command-line flag."""
import functools
import zlib
from fractions import Fraction

import numpy as np
import pytest

import png_cases as pc
import png_deflate_oracle as fixed_ora
import png_dynamic_oracle as ora
import ra_native as rn
import ra_ops as ops
from utils import png


def _raw(img):
  """The scanline bytes zlib.decompress must return: what encode_gray8 / encode_colour8 hand to zlib.compress."""
  img = np.asarray(img)
  rows = (img[:, :, ::-1] if img.ndim == 3 else img).reshape(img.shape[0], -1)
  return np.concatenate([np.zeros((img.shape[0], 1), np.uint8), rows], axis=1).tobytes()


def _bpp(img):
  return 3 if np.asarray(img).ndim == 3 else 1


def _check_batch(imgs):
  """imgs: images of one shape.  The host entry's streams against the restatement, zlib, the Adler-32, the bound and wrap()."""
  batch = np.stack(imgs)
  streams, adler = ops.png_deflate_host(batch, code='dynamic')
  H, W, bpp = batch.shape[1], batch.shape[2], _bpp(imgs[0])
  bound = ora.stream_bound(H, W, bpp)
  assert ops.png_deflate_bound(len(imgs), H, W, bpp, code='dynamic')[0] == bound
  for img, z, a in zip(imgs, streams, adler):
    raw = _raw(img)
    assert z == ora.stream(img)
    assert zlib.decompress(z) == raw
    assert int(a) == zlib.adler32(raw) == int.from_bytes(z[-4:], 'big')
    assert len(z) <= bound, (len(z), bound)
    if bpp == 3:
      assert np.array_equal(png.decode_colour8(png.wrap(H, W, 2, z)), img)
    else:
      assert np.array_equal(png.decode_gray8(png.wrap(H, W, 0, z)), img)
  return streams


@pytest.mark.parametrize('case', pc.grid(), ids=lambda c: c[0])
def test_host_stream_against_zlib_and_restatement(case):
  _, kind, W, named = case
  for H in pc.HEIGHTS:
    imgs = [img for name, img in named if name.endswith('-H%d' % H)]
    assert len(imgs) == (5 if kind == 'colour' else 4)
    _check_batch(imgs)


@pytest.mark.parametrize('case', pc.run_images(), ids=lambda c: c[0])
def test_every_run_length(case):
  _check_batch([case[2]])


def test_white_row_adler_chunk():
  _check_batch([pc.white_row()])


# ---- the limiter alone
def _fib_counts(k, n):
  counts = np.zeros((n,), np.uint32)
  counts[:k] = ora.fibonacci(k)
  return counts


def _spread(counts, seed):
  """the same counts at shuffled symbol indices: ties are broken by index, so the order matters"""
  out = np.array(counts)
  np.random.RandomState(seed).shuffle(out)
  return out


LIMITER_CASES = [
    ('two symbols', np.array([0, 5, 0, 0, 9, 0], np.uint32), 15, None),
    ('all 286 equal', np.full((286,), 7, np.uint32), 15, None),
    ('fibonacci 24 of 286', _fib_counts(24, 286), 15, 23),
    ('fibonacci 40 of 286', _fib_counts(40, 286), 15, 39),
    ('fibonacci 40 of 286, shuffled', _spread(_fib_counts(40, 286), 3), 15, 39),
    ('fibonacci 12 of 19', _fib_counts(12, 19), 7, 11),
    ('fibonacci 12 of 19, shuffled', _spread(_fib_counts(12, 19), 4), 7, 11),
    ('counts of 2^31 - 1', np.full((286,), 2 ** 31 - 1, np.uint32), 15, None),
    ('counts of 2^31 - 1 and ones', np.concatenate([np.full((143,), 2 ** 31 - 1), np.ones((143,))]).astype(np.uint32), 15, None),
]


@pytest.mark.parametrize('case', LIMITER_CASES, ids=lambda c: c[0])
def test_limiter_against_the_restatement(case):
  _, counts, limit, unlimited = case
  if unlimited is not None:
    assert ora.unlimited_depth(counts.tolist()) == unlimited > limit  # the case does need the limiter
  got = ops.png_huffman_lengths(counts, limit).tolist()
  assert got == ora.limited_lengths(counts.tolist(), limit)
  assert max(got) <= limit
  assert all((k > 0) == (c > 0) for k, c in zip(got, counts.tolist()))
  assert sum(Fraction(1, 2 ** k) for k in got if k) == 1  # Kraft: the code is complete


def test_limiter_refusals():
  lib = rn.lib()
  counts, lengths = np.ones((19,), np.uint32), np.full((286,), 0xAB, np.uint8)
  for args, code, word in (((None, 19, 7, rn.ptr(lengths)), 'RA_E_INVALID', 'NULL'), ((rn.ptr(counts), 19, 7, None), 'RA_E_INVALID', 'NULL'),
                           ((rn.ptr(counts), 19, 8, rn.ptr(lengths)), 'RA_E_INVALID', 'limit'),
                           ((rn.ptr(counts), 0, 7, rn.ptr(lengths)), 'RA_E_SHAPE', 'n='),
                           ((rn.ptr(counts), 287, 15, rn.ptr(lengths)), 'RA_E_SHAPE', 'n='),
                           ((rn.ptr(counts), 129, 7, rn.ptr(lengths)), 'RA_E_SHAPE', 'n=')):
    assert lib.ra_png_huffman_lengths(*args) == getattr(rn, code)
    assert word in lib.ra_last_error_string().decode()
    assert (lengths == 0xAB).all()


# ---- the limit through the whole path
@functools.lru_cache(maxsize=None)
def _forced():
  img = ora.forced_limit_image()
  rows, d = fixed_ora.scanlines(img)
  return img, ora.histogram(rows, d)


def test_forced_limit_image():
  img, hist = _forced()
  assert img.shape == (1991, 61)
  assert ora.unlimited_depth(hist) > 15  # the image does force the limit ...
  assert max(ora.limited_lengths(hist, 15)) <= 15 < ora.unlimited_depth(hist)
  _check_batch([img])


# ---- edge cases
def test_one_pixel():
  for img in (np.zeros((1, 1), np.uint8), np.full((1, 1), 255, np.uint8), np.array([[[1, 2, 3]]], np.uint8)):
    z = _check_batch([img])[0]
    assert len(z) <= ora.stream_bound(1, 1, _bpp(img))


def test_no_match_at_all():
  """Rows without three equal bytes in a row at distance d: the distance code is declared (HDIST, one length) and never used."""
  for kind in pc.KINDS:
    img = pc.alternating(kind, 5, 37)
    rows, d = fixed_ora.scanlines(img)
    assert all(k == 'lit' for r in rows for k, _ in fixed_ora.tokens(r, d))
    _check_batch([img])


def test_float_source_and_plane_list():
  """float32 planes quantised in the load as (y * 255).to(uint8), among them 0, 0.5, 1 - 2^-24 and 1, picked by a list that
  skips, repeats and reorders."""
  y = np.zeros((5, 6, 70), np.float32)
  y[0] = 1.0
  y[1] = 0.5
  y[2] = np.resize(np.array([0.0, 0.5, 1.0 - 2.0 ** -24, 1.0], np.float32), (6, 70))
  y[3] = np.float32(1.0 - 2.0 ** -24)
  y[4] = np.random.RandomState(3).rand(6, 70) > 0.5
  assert y[3, 0, 0] < 1.0
  want = (y * np.float32(255.0)).astype(np.uint8)
  assert want[1, 0, 0] == 127 and want[0, 0, 0] == 255 and want[4].max() == 255 and want[4].min() == 0
  planes = [4, 0, 0, 3, 1]  # skips 2, repeats 0, out of order
  streams, _ = ops.png_deflate_host(y, planes, code='dynamic')
  assert len(streams) == len(planes)
  for p, z in zip(planes, streams):
    assert zlib.decompress(z) == _raw(want[p])
    assert z == ora.stream(want[p])
  full, _ = ops.png_deflate_host(y, code='dynamic')
  assert full == [ora.stream(w) for w in want]
  grey = np.random.RandomState(8).randint(0, 2, size=(4, 3, 19)).astype(np.uint8) * 255
  picked, _ = ops.png_deflate_host(grey, [3, 1, 1, 0], code='dynamic')
  assert picked == [ora.stream(grey[p]) for p in (3, 1, 1, 0)]


# ---- the grid reaches what the placement has to handle
def test_grid_covers_every_row_alignment():
  """Over the grid the rows start at every bit offset mod 32, some rows cross a dword boundary, some dwords hold the starts of
  several rows (rows shorter than a dword), and a row ends exactly on a dword boundary or the bit before or after it."""
  starts_mod, crosses, shared, ends_mod = set(), 0, 0, set()
  for _, kind, W, named in pc.grid():
    for _, img in named:
      places = ora.row_places(img)
      starts_mod.update(s % 32 for s in places[:-1])
      ends_mod.update(e % 32 for e in places[1:])
      crosses += sum(1 for s, e in zip(places[:-1], places[1:]) if s // 32 != (e - 1) // 32)
      per_dword = {}
      for s in places[:-1]:
        per_dword[s // 32] = per_dword.get(s // 32, 0) + 1
      shared += sum(1 for v in per_dword.values() if v >= 3)
  assert starts_mod == set(range(32)), sorted(set(range(32)) - starts_mod)
  assert ends_mod >= {31, 0, 1}
  assert crosses > 100 and shared > 10, (crosses, shared)


# ---- size
def test_smaller_than_the_fixed_format():
  yy, xx = np.mgrid[0:64, 0:96]
  disc = (((xx - 48) ** 2 + (yy - 32) ** 2) < 20 ** 2).astype(np.uint8) * 255
  flat = np.zeros((7, 33, 3), np.uint8)
  flat[:, 5:20] = (43, 57, 192)
  flat[2:5, 12:30] = (18, 156, 243)
  for img in (disc, flat):
    dyn = _check_batch([img])[0]
    fix = ops.png_deflate_host(img[None])[0][0]
    assert zlib.decompress(fix) == zlib.decompress(dyn)
    assert len(dyn) < len(fix), (len(dyn), len(fix))


def test_bound_query():
  import ctypes
  lib = rn.lib()
  a, b = ctypes.c_ulonglong(5), ctypes.c_ulonglong(6)
  for args, word in (((1, 2, 4, 2), 'bpp'), ((0, 2, 4, 1), 'N='), ((1, 0, 4, 1), 'H='), ((1, 2, 0, 1), 'W='),
                     ((1, 1, 8192, 3), 'scanlines'), ((1, 90000, 24575, 1), '2^31')):
    assert lib.ra_png_deflate_dyn_bound(*args, ctypes.addressof(a), ctypes.addressof(b)) == rn.RA_E_SHAPE
    msg = lib.ra_last_error_string().decode()
    assert word in msg and 'ra_png_deflate_dyn_bound' in msg
    assert (a.value, b.value) == (5, 6)
  assert lib.ra_png_deflate_dyn_bound(1, 2, 4, 1, None, ctypes.addressof(b)) == rn.RA_E_INVALID
  for N, H, W, bpp in ((1, 1, 1, 1), (20, 1024, 2048, 1), (1, 1024, 2048, 3), (3, 7, 1031, 3)):
    stream, ws = ops.png_deflate_bound(N, H, W, bpp, code='dynamic')
    n = 1 + W * bpp
    assert stream == 270 + -(-15 * n * H // 8) == ora.stream_bound(H, W, bpp)
    assert ws >= N * (288 * 4 + H * (16 + 8 + -(-15 * n // 8)))  # a histogram per image; a record, a place and a slot per row


# ---- refusals: the code by name, the message naming the argument, the outputs untouched
def _call(fn, src, kind, M, N, H, W, out_bytes=None, plane=None, null=(), ws=None, ws_bytes=0):
  bpp = 3 if kind == rn.RA_PNG_BGR8 else 1
  cap = 270 + -(-15 * (1 + max(1, W) * bpp) * max(1, H) // 8)
  out = np.full((max(1, N) * min(cap, 1 << 16),), 0xAB, np.uint8)
  sizes, offsets, adler = np.full((8,), -7, np.int32), np.full((8,), 77, np.uint64), np.full((8,), 99, np.uint32)
  args = {'src': rn.ptr(src), 'out': rn.ptr(out), 'sizes': rn.ptr(sizes), 'offsets': rn.ptr(offsets), 'adler': rn.ptr(adler)}
  for k in null:
    args[k] = None
  tail = (ws, ws_bytes) if fn == 'ra_png_deflate_dyn_host' else (ws, ws_bytes, None)
  rc = getattr(rn.lib(), fn)(args['src'], kind, M, N, H, W, rn.ptr(plane), args['out'], out.size if out_bytes is None else out_bytes,
                             args['sizes'], args['offsets'], args['adler'], *tail)
  assert (out == 0xAB).all() and (sizes == -7).all() and (offsets == 77).all() and (adler == 99).all()
  return rc, (rn.lib().ra_last_error_string() or b'').decode()


REFUSALS = [
    # (what, kind, M, N, H, W, keyword arguments, the code, a word of the message): the fixed entries' list
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
    ('capacity one byte short', 0, 1, 1, 2, 4, {'out_bytes': 270 + 19 - 1}, 'RA_E_WORKSPACE', 'out_bytes'),
]


@pytest.mark.parametrize('fn', ['ra_png_deflate_dyn_host', 'ra_png_deflate_dyn_u8'])
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
  ws = np.zeros((8192,), np.uint8)
  need = ops.png_deflate_bound(1, 2, 4, 1, code='dynamic')[1]
  assert need + 32 <= ws.size
  base = rn.ptr(ws) + (-rn.ptr(ws) % 16)
  for what, p, nbytes in (('NULL', None, need), ('short', base, need - 1), ('not aligned', base + 8, need)):
    rc, msg = _call('ra_png_deflate_dyn_u8', src, 0, 1, 1, 2, 4, ws=p, ws_bytes=nbytes)
    assert rc == rn.RA_E_WORKSPACE and 'ws' in msg, (what, rc, msg)


def test_host_entry_refuses_a_plane_index_outside_the_source():
  src = np.zeros((2, 2, 4), np.uint8)
  for bad in (-1, 2):
    rc, msg = _call('ra_png_deflate_dyn_host', src, 0, 2, 2, 2, 4, plane=np.array([0, bad], np.int32))
    assert rc == rn.RA_E_SHAPE and 'plane[1]' in msg, (rc, msg)


# ---- the keyword and the flag
def test_another_code_is_refused_by_name():
  img = np.zeros((1, 2, 3), np.uint8)
  for call in (lambda: ops.png_deflate_host(img, code='huffman'), lambda: ops.png_deflate_bound(1, 2, 3, 1, code='huffman'),
               lambda: ops.png_deflate(img, code='huffman')):
    with pytest.raises(rn.RecAttendError, match='huffman'):
      call()
  import analysis
  with pytest.raises(ValueError, match='huffman'):
    analysis.RenderInstanceAnalyzer('unused', [], device_png=True, device_png_code='huffman')


def test_defaults_keep_the_fixed_format():
  img = (np.random.RandomState(1).rand(2, 5, 40) > 0.7).astype(np.uint8) * 255
  assert ops.png_deflate_host(img)[0] == ops.png_deflate_host(img, code='fixed')[0] == [fixed_ora.stream(i) for i in img]
  assert ops.png_deflate_bound(2, 5, 40, 1) == ops.png_deflate_bound(2, 5, 40, 1, code='fixed')


@pytest.mark.parametrize('module', ['cityscapes_eval', 'full_model_eval', 'fg_model_eval'])
def test_flag_needs_device_png(module):
  """--device_png_code without --device_png is an error that names both flags, raised before any work; the default is fixed."""
  import importlib
  mod = importlib.import_module(module)
  with pytest.raises(ValueError) as e:
    mod.main(['--device_png_code', 'dynamic'])
  assert '--device_png_code' in str(e.value) and '--device_png ' in str(e.value).replace(':', ' ')
  args = mod.build_parser().parse_args(['--device_png'])
  import cmd_args_parser as cap
  assert cap.device_png_code(args) == 'fixed'
  assert cap.device_png_code(mod.build_parser().parse_args(['--device_png', '--device_png_code', 'dynamic'])) == 'dynamic'
  with pytest.raises(SystemExit):
    mod.build_parser().parse_args(['--device_png', '--device_png_code', 'zlib'])
