"""The device PNG encoder's "dynamic" stream format on the MI355X (csrc/ra_png_dyn.hip): its streams, sizes, offsets and Adler-32
against ra_png_deflate_dyn_host byte for byte (which tests/test_png_dynamic.py holds against zlib and the Python restatement) on
the same case grid, with the output and the workspace poisoned before the call; tall images, batches with a plane list, both
load forms, the float source, the image that forces the length limit, two streams, and the Cityscapes output stage end to end."""
import os
import zlib

import numpy as np
import pytest
import torch

import png_cases as pc
import png_dynamic_oracle as ora
import ra_native as rn
import ra_ops as ops
from utils import png

pytestmark = pytest.mark.gpu


def _raw(img):
  img = np.asarray(img)
  rows = (img[:, :, ::-1] if img.ndim == 3 else img).reshape(img.shape[0], -1)
  return np.concatenate([np.zeros((img.shape[0], 1), np.uint8), rows], axis=1).tobytes()


def _device_poisoned(src, plane_index=None):
  """ONE ra_png_deflate_dyn_u8 call on the device tensor src, `out` and the workspace filled with 0xAB before: a chain that relies
  on a cleared buffer fails.  -> (streams, sizes, offsets, adler)"""
  kind, M, H, W, bpp = ops._png_source('test', src)
  idx = None if plane_index is None else torch.tensor(plane_index, dtype=torch.int32, device='cuda')
  N = M if idx is None else int(idx.numel())
  stream, ws_bytes = ops.png_deflate_bound(N, H, W, bpp, code='dynamic')
  out = torch.full((N * stream,), 0xAB, dtype=torch.uint8, device='cuda')
  ws = torch.full((ws_bytes,), 0xAB, dtype=torch.uint8, device='cuda')
  sizes = torch.full((N,), -7, dtype=torch.int32, device='cuda')
  offsets = torch.full((N,), -7, dtype=torch.int64, device='cuda')
  adler = torch.full((N,), -7, dtype=torch.int32, device='cuda')
  rn.check(rn.lib().ra_png_deflate_dyn_u8(rn.ptr(src), kind, M, N, H, W, rn.ptr(idx), rn.ptr(out), out.numel(), rn.ptr(sizes),
                                          rn.ptr(offsets), rn.ptr(adler), rn.ptr(ws), ws.numel(), rn.stream_ptr()), 'ra_png_deflate_dyn_u8')
  data, sizes, offsets = out.cpu().numpy(), sizes.cpu().numpy().astype(np.int64), offsets.cpu().numpy()
  streams = [data[int(o):int(o) + int(n)].tobytes() for n, o in zip(sizes, offsets)]
  used = int(offsets[-1] + sizes[-1])
  assert (data[used:] == 0xAB).all(), 'bytes behind the last stream were written'
  return streams, sizes, offsets, adler.cpu().numpy().view(np.uint32)


def _device_equals_host(batch, plane_index=None):
  """batch: a NumPy array of one of the three source kinds; returns the streams."""
  want, adler = ops.png_deflate_host(batch, plane_index, code='dynamic')
  got, sizes, offsets, dev_adler = _device_poisoned(torch.from_numpy(batch).cuda(), plane_index)
  assert sizes.tolist() == [len(z) for z in want]
  assert offsets.tolist() == np.concatenate([[0], np.cumsum(sizes)[:-1]]).tolist()
  assert dev_adler.tolist() == adler.tolist()
  for k, (g, w) in enumerate(zip(got, want)):
    assert g == w, 'image %d: the device stream differs from the host stream' % k
  return got


@pytest.mark.parametrize('case', pc.grid(), ids=lambda c: c[0])
def test_device_stream_is_the_host_stream(cuda, case):
  _, kind, W, named = case
  for H in pc.HEIGHTS:
    _device_equals_host(np.stack([img for name, img in named if name.endswith('-H%d' % H)]))


@pytest.mark.parametrize('case', pc.run_images(), ids=lambda c: c[0])
def test_every_run_length(cuda, case):
  _device_equals_host(case[2][None])


def test_white_row_adler_chunk(cuda):
  z = _device_equals_host(pc.white_row()[None])[0]
  assert int.from_bytes(z[-4:], 'big') == zlib.adler32(_raw(pc.white_row()))


@pytest.mark.parametrize('H', [1, 2, 7, 257, 513])
def test_tall_images(cuda, H):
  """The row scan in one pass of its 256 threads, at the edge of it and in three passes; rows of a few bits and of a few dwords."""
  rs = np.random.RandomState(H)
  for W in (3, 150):
    imgs = [(rs.rand(H, W) > 0.8).astype(np.uint8) * 255, np.zeros((H, W), np.uint8), rs.randint(0, 256, size=(H, W)).astype(np.uint8)]
    for z, img in zip(_device_equals_host(np.stack(imgs)), imgs):
      assert zlib.decompress(z) == _raw(img)


@pytest.mark.parametrize('kind', pc.KINDS)
def test_batch_with_a_plane_list_and_both_load_forms(cuda, kind):
  """N = 3 of M = 4 with a reordering plane list; the same pixels from a view that is not 16-byte aligned (element loads) and from
  an aligned one with W % 16 == 0 (16-byte loads) give the same bytes, through ra_ops.png_deflate as well."""
  rs = np.random.RandomState(23)
  c = () if kind == 'grey' else (3,)
  whole = (rs.rand(4, 9, 64, *c) > 0.8).astype(np.uint8) * 255
  whole[3] = rs.randint(0, 256, size=whole[3].shape)
  got = _device_equals_host(whole, [2, 0, 3])
  assert [zlib.decompress(z) for z in got] == [_raw(whole[p]) for p in (2, 0, 3)]
  flat = torch.zeros((whole.size + 16,), dtype=torch.uint8, device='cuda')
  want, _ = ops.png_deflate_host(whole, code='dynamic')
  for shift in (0, 1, 4, 8):
    flat[shift:shift + whole.size] = torch.from_numpy(whole).cuda().reshape(-1)
    view = flat[shift:shift + whole.size].view(*whole.shape)
    assert view.data_ptr() % 16 == shift and view.is_contiguous()
    assert _device_poisoned(view)[0] == want
    assert ops.png_deflate(view, code='dynamic') == want
  odd = (rs.rand(3, 7, 33, *c) > 0.5).astype(np.uint8) * 255  # odd H * W: the second image starts at an odd address
  _device_equals_host(odd)


def test_float_source_with_a_plane_list(cuda):
  for W in (70, 64):  # element loads / 16-byte loads
    y = np.zeros((6, 5, W), np.float32)
    y[0], y[1], y[3] = 1.0, 0.5, np.float32(1.0 - 2.0 ** -24)
    y[2] = np.resize(np.arange(256, dtype=np.float32) / np.float32(255.0), (5, W))
    y[4] = np.random.RandomState(3).rand(5, W) > 0.5
    y[5] = np.resize(np.array([0.0, 0.5, 1.0 - 2.0 ** -24, 1.0], np.float32), (5, W))
    dev = torch.from_numpy(y).cuda()
    want = (dev * 255).to(torch.uint8).cpu().numpy()  # the analyzer's own expression
    assert np.array_equal(want, (y * np.float32(255.0)).astype(np.uint8))
    planes = [5, 0, 0, 3, 1, 2]  # skips 4, repeats 0, out of order
    got = _device_equals_host(y, planes)
    for p, z in zip(planes, got):
      assert zlib.decompress(z) == _raw(want[p])
    assert [zlib.decompress(z) for z in ops.png_deflate(dev[1:], [3, 3], code='dynamic')] == [_raw(want[4])] * 2  # a view at an offset


def test_forced_limit_image(cuda):
  img = ora.forced_limit_image()
  z = _device_equals_host(img[None])[0]
  assert zlib.decompress(z) == _raw(img)


def test_longest_row(cuda):
  """One scanline of RA_PNG_MAX_ROW_BYTES bytes of noise: the encode kernel's largest LDS request (above 64 KiB)."""
  img = np.random.RandomState(9).randint(0, 256, size=(2, rn.RA_PNG_MAX_ROW_BYTES - 1)).astype(np.uint8)
  assert zlib.decompress(_device_equals_host(img[None])[0]) == _raw(img)


def test_two_streams_give_equal_bytes(cuda):
  rs = np.random.RandomState(31)
  src = torch.from_numpy((rs.rand(3, 40, 300) > 0.9).astype(np.uint8) * 255).cuda()
  torch.cuda.synchronize()
  got = []
  for _ in range(2):
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
      got.append(ops.png_deflate(src, code='dynamic'))
    st.synchronize()
  assert got[0] == got[1] == ops.png_deflate_host(src.cpu().numpy(), code='dynamic')[0]
  assert got[0] != ops.png_deflate(src)  # the default is the other format


def test_cityscapes_output_stage_end_to_end(cuda, tmp_path):
  """A 2-image, T = 3, 32 x 64 batch through RenderCityScapesOutputAnalyzer with the host writer, the fixed and the dynamic device
  format: the same text, the same pixels in every mask file, and the dynamic files are the smallest of the device's."""
  import analysis
  rs = np.random.RandomState(41)
  yy, xx = np.mgrid[0:32, 0:64]
  y = np.stack([np.stack([((xx - rs.randint(10, 54)) ** 2 + (yy - rs.randint(8, 24)) ** 2 < rs.randint(4, 12) ** 2) for _ in range(3)])
                for _ in range(2)]).astype(np.float32)
  names = ['aachen_000001_000019.png', 'bochum_000002_000019.png']

  def run(folder, **kw):
    res = {'y_out': torch.from_numpy(y).cuda(), 'conf': torch.full((2, 3), 0.9, device='cuda'), 'indices': [0, 1],
           '_instance_class': (torch.zeros((2, 3), dtype=torch.int32, device='cuda'),
                               torch.full((2, 3), 26, dtype=torch.int32, device='cuda'), None)}
    an = analysis.RenderCityScapesOutputAnalyzer(str(tmp_path / folder), names, **kw)
    an.stage(res)
    return an.written

  host = run('host')
  fixed = run('fixed', device_png=True)
  dyn = run('dyn', device_png=True, device_png_code='dynamic')
  n = 0
  for (th, lh), (tf, lf), (td, ld) in zip(host, fixed, dyn):
    assert lh == lf == ld and len(lh) == 3
    assert open(th).read() == open(td).read()
    for k, (img_file, _, _) in enumerate(lh):
      ph, pf, pd = (os.path.join(os.path.dirname(t), img_file) for t in (th, tf, td))
      ii = names.index(os.path.basename(th)[:-4] + '.png')
      want = (y[ii, k] * 255).astype(np.uint8)
      assert np.array_equal(png.read_gray8(ph), want) and np.array_equal(png.read_gray8(pd), want)
      assert np.array_equal(png.read_gray8(pf), want)
      assert os.path.getsize(pd) < os.path.getsize(pf)
      n += 1
  assert n == 6
