"""The ragged PNG encoder on the MI355X (csrc/ra_png.hip, csrc/ra_png_dyn.hip instantiated over the ragged geometry): its streams
against ra_png_deflate*_ragged_host byte for byte on the batches of tests/png_ragged_cases.py (where tests/test_png_ragged.py
holds the host entries against the uniform entry of every image alone and against zlib), with the output and the workspace
poisoned before the call; the three layouts; repeated runs; the uniform device entry on a one-image batch; the longest scanline;
the float source with a plane list; a refused table."""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

import png_ragged_cases as rc
import ra_native as rn
import ra_ops as ops

pytestmark = pytest.mark.gpu

PLANES = [3, 0, 0, 2]


def _poison(dev):
  """The wrapper's reusable workspace and output buffers, and everything cached free, filled with 0xA5."""
  for t in ops._PNG_BUFFERS.get(str(dev), []):
    if t is not None:
      t.fill_(0xA5)


def _device(src, geo, plane_index=None, code='fixed'):
  """One ragged device call on poisoned buffers -> (streams, sizes, offsets, adler)."""
  t = torch.from_numpy(src).cuda()
  ops.png_deflate_ragged(t, geo, plane_index, code=code)  # sizes the wrapper's buffers for this call
  _poison(t.device)
  return ops.png_deflate_ragged(t, geo, plane_index, with_meta=True, code=code)


def _device_equals_host(src, geo, plane_index=None, code='fixed'):
  want, wsizes, woffsets, wadler = ops.png_deflate_ragged_host(src, geo, plane_index, code=code)
  got, sizes, offsets, adler = _device(src, geo, plane_index, code)
  assert sizes.tolist() == wsizes.tolist()
  assert offsets.tolist() == woffsets.tolist() == np.concatenate([[0], np.cumsum(sizes)[:-1]]).tolist()
  assert adler.tolist() == wadler.tolist()
  for i, (g, w) in enumerate(zip(got, want)):
    assert g == w, 'stream %d: the device stream differs from the host stream' % i
  return got


@pytest.mark.parametrize('batch', rc.BATCHES)
@pytest.mark.parametrize('kind', rc.KINDS)
@pytest.mark.parametrize('code', rc.CODES)
def test_device_is_the_ragged_host_and_layouts_agree(cuda, code, kind, batch):
  """Every layout against the host entry; and, put back into the images' order, the three layouts give identical streams."""
  per_layout = []
  for name, _, _ in rc.LAYOUTS:
    src, geo, order = rc.layout(batch, kind, name)
    got = _device_equals_host(src, geo, code=code)
    B = len(order)
    assert got == [z for z, _ in rc.expected(batch, kind, code, order)]
    per_layout.append([[got[k * B + order.index(j)] for j in range(B)] for k in range(len(src))])
  assert per_layout[0] == per_layout[1] == per_layout[2]


@pytest.mark.parametrize('kind', rc.KINDS)
@pytest.mark.parametrize('code', rc.CODES)
def test_plane_list_and_two_runs_are_bit_identical(cuda, code, kind):
  """plane = [3, 0, 0, 2] of the mixed batch (the float source included), twice."""
  src, geo, order = rc.layout('mixed', kind, 'align4')
  first = _device_equals_host(src, geo, PLANES, code)
  assert first == [z for z, _ in rc.expected('mixed', kind, code, order, PLANES)]
  again, sizes, offsets, adler = _device(src, geo, PLANES, code)
  assert again == first


@pytest.mark.parametrize('code', rc.CODES)
def test_one_image_batch_is_the_uniform_device_entry(cuda, code):
  rs = np.random.RandomState(5)
  for shape in ((9, 64), (9, 70), (9, 64, 3), (5, 33, 3)):
    img = (rs.rand(*shape) > 0.7).astype(np.uint8) * 255
    geo, total = ops.ragged_geometry([shape[:2]], 1)
    flat = torch.from_numpy(img.reshape((1, total) + shape[2:])).cuda()
    got, sizes, offsets, adler = ops.png_deflate_ragged(flat, geo, with_meta=True, code=code)
    want, usizes, uoffsets, uadler = ops.png_deflate(torch.from_numpy(img[None]).cuda(), with_meta=True, code=code)
    assert got == want and sizes.tolist() == usizes.tolist() and offsets.tolist() == uoffsets.tolist()
    assert adler.tolist() == uadler.tolist()


def test_longest_scanline_beside_one_pixel(cuda):
  """One grey row of 24575 pixels — RA_PNG_MAX_ROW_BYTES with its filter byte; the dynamic format's encode kernel then takes more
  than 64 KiB of LDS, the opt-in of its ragged instantiation — beside a 1 x 1 image, in both orders."""
  W = rn.RA_PNG_MAX_ROW_BYTES - 1
  rs = np.random.RandomState(11)
  row = np.repeat(rs.randint(0, 256, size=(1, W // 3 + 1)), 3, axis=1)[:, :W].astype(np.uint8)
  row[0, ::7] = rs.randint(0, 256, size=row[0, ::7].shape)
  dot = np.full((1, 1), 200, np.uint8)
  for imgs in ((row, dot), (dot, row)):
    geo, total = ops.ragged_geometry([i.shape for i in imgs], 1)
    src = np.concatenate([i.reshape(-1) for i in imgs])[None]
    for code in rc.CODES:
      got = _device_equals_host(src, geo, code=code)
      for img, z in zip(imgs, got):
        assert zlib.decompress(z) == rc.scanlines(img)
        assert z == ops.png_deflate_host(img[None], code=code)[0][0]


def test_refused_table_leaves_the_outputs_untouched(cuda):
  """The device entry itself with an overlapping table and with a scanline that is too long: RA_E_SHAPE, the image named, and
  out, sizes, offsets, adler, the device table and the workspace as they were — nothing was launched."""
  dev = torch.device('cuda')
  for code in rc.CODES:
    fn = getattr(rn.lib(), ops.PNG_CODES[code] + '_ragged_u8')
    for rows, word in (([(0, 2, 5), (9, 3, 4)], 'inside image 0'), ([(0, 2, 5), (12, 1, rn.RA_PNG_MAX_ROW_BYTES)], 'scanlines')):
      tab = (rn.ImageGeo * 2)(*[rn.ImageGeo(*r) for r in rows])
      src = torch.zeros((1 << 16,), dtype=torch.uint8, device=dev)
      bufs = [torch.full((n,), 0xA5, dtype=torch.uint8, device=dev) for n in (1 << 16, 64, 64, 64, 64, 1 << 20)]
      out, sizes, offsets, adler, gdev, ws = bufs
      got = fn(rn.ptr(src), rn.RA_PNG_GRAY8, 1, src.numel(), tab, rn.ptr(gdev), 2, None, 1, rn.ptr(out), out.numel(), rn.ptr(sizes),
               rn.ptr(offsets), rn.ptr(adler), rn.ptr(ws), ws.numel(), rn.stream_ptr())
      msg = rn.lib().ra_last_error_string().decode()
      assert got == rn.RA_E_SHAPE and 'image 1' in msg and word in msg, (got, msg)
      torch.cuda.synchronize()
      for t in bufs:
        assert bool((t == 0xA5).all())
