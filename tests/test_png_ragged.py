"""The ragged PNG encoder without a device: ra_png_deflate_ragged_host / ra_png_deflate_dyn_ragged_host against the uniform host
entry of every image alone (byte for byte) and against zlib.decompress, in every layout of tests/png_ragged_cases.py; the bound;
every refusal by name; analysis.RaggedPicture as the list of views it replaces."""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

import png_ragged_cases as rc
import ra_native as rn
import ra_ops as ops

PLANES = [3, 0, 0, 2]  # skips 1, repeats 0, reorders


def _check_call(batch, kind, code, name, plane_index=None):
  src, geo, order = rc.layout(batch, kind, name)
  streams, sizes, offsets, adler = ops.png_deflate_ragged_host(src, geo, plane_index, code=code)
  want = rc.expected(batch, kind, code, order, plane_index)
  assert len(streams) == len(want) == (len(src) if plane_index is None else len(plane_index)) * len(order)
  assert sizes.tolist() == [len(z) for z in streams]
  assert offsets.tolist() == np.concatenate([[0], np.cumsum(sizes.astype(np.int64))[:-1]]).tolist()
  ps = rc.planes(batch, kind)
  ks = range(len(ps)) if plane_index is None else plane_index
  imgs = [ps[k][j] for k in ks for j in order]
  for i, (z, a, (wz, wa), img) in enumerate(zip(streams, adler, want, imgs)):
    assert z == wz, 'stream %d differs from the uniform host entry of its image alone' % i
    raw = rc.scanlines(img)
    assert zlib.decompress(z) == raw
    assert int(a) == wa == zlib.adler32(raw) == int.from_bytes(z[-4:], 'big')
  return streams


@pytest.mark.parametrize('name', [l[0] for l in rc.LAYOUTS])
@pytest.mark.parametrize('batch', rc.BATCHES)
@pytest.mark.parametrize('kind', rc.KINDS)
@pytest.mark.parametrize('code', rc.CODES)
def test_ragged_host_is_the_uniform_host_per_image(code, kind, batch, name):
  _check_call(batch, kind, code, name)


@pytest.mark.parametrize('name', [l[0] for l in rc.LAYOUTS])
@pytest.mark.parametrize('kind', rc.KINDS)
@pytest.mark.parametrize('code', rc.CODES)
def test_plane_list_skips_repeats_and_reorders(code, kind, name):
  src, _, order = rc.layout('mixed', kind, name)
  assert len(src) >= 4
  streams = _check_call('mixed', kind, code, name, PLANES)
  B = len(order)
  assert streams[B:2 * B] == streams[2 * B:3 * B]  # plane 0 twice


def test_one_plane_sources_are_M_1():
  for kind in rc.KINDS:
    src, geo, order = rc.layout('runs', kind, 'align4')
    assert len(src) == 1
    got = ops.png_deflate_ragged_host(src[0], geo)[0]
    assert got == [z for z, _ in rc.expected('runs', kind, 'fixed', order)]


# ---- the bound and the refusals: the C entries themselves ------------------------------------------------------------------
def _table(rows):
  return (rn.ImageGeo * len(rows))(*[rn.ImageGeo(int(o), int(h), int(w)) for o, h, w in rows])


def _bound(code, rows, Np, bpp):
  out, ws = C.c_ulonglong(0), C.c_ulonglong(0)
  fn = getattr(rn.lib(), ops.PNG_CODES[code] + '_ragged_bound')
  rc_ = fn(_table(rows), len(rows), Np, bpp, C.addressof(out), C.addressof(ws))
  return rc_, int(out.value), int(ws.value)


@pytest.mark.parametrize('code', rc.CODES)
@pytest.mark.parametrize('bpp', (1, 3))
def test_bound_is_the_sum_of_the_images_bounds(code, bpp):
  geo, _ = ops.ragged_geometry(rc.MIXED, 4)
  each = [ops.png_deflate_bound(1, h, w, bpp, code) for h, w in rc.MIXED]
  for Np in (1, 3):
    out, ws = ops.png_deflate_ragged_bound(geo, Np, bpp, code)
    assert out == Np * sum(s for s, _ in each)
    # the workspace is the uniform entry's for Np * B images of the tallest and the widest image of the batch
    assert ws == ops.png_deflate_bound(Np * len(rc.MIXED), max(h for h, _ in rc.MIXED), max(w for _, w in rc.MIXED), bpp, code)[1]


class _Call(object):
  """A call of a ragged entry on small host buffers, every argument replaceable; out, sizes, offsets and adler are poisoned
  and must come back untouched from a refusal."""

  def __init__(self, code, device=False):
    self.name = ops.PNG_CODES[code] + ('_ragged_u8' if device else '_ragged_host')
    self.device = device
    self.rows = [(0, 2, 5), (12, 3, 4)]
    self.total, self.M, self.kind = 24, 2, rn.RA_PNG_GRAY8
    self.src = np.zeros((self.M * self.total,), np.uint8)
    self.plane, self.Np = None, 2
    self.out_bytes = _bound(code, self.rows, 2, 1)[1]
    self.ws, self.ws_bytes = None, 0

  def run(self, null=()):
    tab = _table(self.rows)
    out = np.full((max(self.out_bytes, 1),), 0xA5, np.uint8)
    N = max(len(self.rows) * max(self.Np, 1), 1)
    N = min(N, 1 << 17)
    sizes, offsets, adler = np.full((N,), -7, np.int32), np.full((N,), 77, np.uint64), np.full((N,), 777, np.uint32)
    p = {'src': rn.ptr(self.src), 'geo': tab, 'out': rn.ptr(out), 'sizes': rn.ptr(sizes), 'offsets': rn.ptr(offsets),
         'adler': rn.ptr(adler), 'geo_dev': 16}
    for k in null:
      p[k] = None
    plane = None if self.plane is None else np.asarray(self.plane, np.int32)
    args = [p['src'], self.kind, self.M, self.total, p['geo']] + ([p['geo_dev']] if self.device else []) + [
        len(self.rows), rn.ptr(plane), self.Np, p['out'], self.out_bytes, p['sizes'], p['offsets'], p['adler'], self.ws, self.ws_bytes]
    code = getattr(rn.lib(), self.name)(*(args + ([None] if self.device else [])))
    assert (out == 0xA5).all() and (sizes == -7).all() and (offsets == 77).all() and (adler == 777).all() or code == 0
    return code, (rn.lib().ra_last_error_string() or b'').decode()


def _refused(call, code, *words, **kw):
  got, msg = call.run(**kw)
  assert got == code, (got, msg)
  for w in (call.name,) + words:
    assert w in msg, (w, msg)


@pytest.mark.parametrize('code', rc.CODES)
def test_a_capacity_one_byte_short_is_refused_and_out_untouched(code):
  c = _Call(code)
  assert c.run()[0] == 0
  c.out_bytes -= 1
  _refused(c, rn.RA_E_WORKSPACE, 'out_bytes=%d' % c.out_bytes)


@pytest.mark.parametrize('code', rc.CODES)
def test_every_refusal_names_its_image_or_argument(code):
  def call(**kw):
    c = _Call(code)
    for k, v in kw.items():
      setattr(c, k, v)
    return c
  # the table: sizes, order, overlap, the buffer's end
  _refused(call(rows=[(0, 2, 5), (12, 0, 4)]), rn.RA_E_SHAPE, 'image 1', '0 x 4')
  _refused(call(rows=[(0, 2, 5), (12, 3, -1)]), rn.RA_E_SHAPE, 'image 1')
  _refused(call(rows=[(0, 2, 5), (9, 3, 4)]), rn.RA_E_SHAPE, 'image 1', 'inside image 0')
  _refused(call(rows=[(0, 2, 5), (13, 3, 4)]), rn.RA_E_SHAPE, 'image 1', 'beyond')
  # the per-image limits of the uniform entries (refused before anything is read: the buffers stay small)
  wide = rn.RA_PNG_MAX_ROW_BYTES
  _refused(call(rows=[(0, 2, 5), (12, 1, wide)], total=1 << 40), rn.RA_E_SHAPE, 'image 1', 'scanlines of %d bytes' % (wide + 1))
  _refused(call(rows=[(0, 1, 8192), (8192, 1, 8192)], total=1 << 40, kind=rn.RA_PNG_BGR8), rn.RA_E_SHAPE, 'image 0', 'scanlines')
  _refused(call(rows=[(0, 2, 5), (12, 32768, 16384)], total=1 << 40, kind=rn.RA_PNG_F32), rn.RA_E_SHAPE, 'image 1', 'source bytes')
  _refused(call(rows=[(0, 2, 5), (12, 90000, 22000)], total=1 << 40), rn.RA_E_SHAPE, 'image 1', 'a stream of up to')
  _refused(call(rows=[(0, 2, 5), (12, 1 << 16, 1 << 15)], total=1 << 40), rn.RA_E_SHAPE, 'image 1')
  # the counts
  _refused(call(Np=0), rn.RA_E_SHAPE, 'Np=0')
  _refused(call(Np=rn.RA_PNG_MAX_IMAGES // 2 + 1, plane=[0]), rn.RA_E_SHAPE, 'N = Np * B <= %d' % rn.RA_PNG_MAX_IMAGES)
  _refused(call(M=0), rn.RA_E_SHAPE, 'M=0')
  _refused(call(Np=3), rn.RA_E_SHAPE, 'Np=3', 'M=2', 'without a plane list')
  _refused(call(plane=[1, 2]), rn.RA_E_SHAPE, 'plane[1]=2')
  _refused(call(plane=[-1, 0]), rn.RA_E_SHAPE, 'plane[0]=-1')
  # pointers and the kind
  for arg in ('src', 'geo', 'out', 'sizes', 'offsets', 'adler'):
    _refused(call(), rn.RA_E_INVALID, 'NULL', null=(arg,))
  _refused(call(kind=3), rn.RA_E_INVALID, 'kind 3')
  # the device entry's own: refused before its first GPU call, so this runs without a device
  dev = _Call(code, device=True)
  _refused(dev, rn.RA_E_INVALID, 'geo_dev', null=('geo_dev',))
  _refused(dev, rn.RA_E_WORKSPACE, 'ws=')  # NULL
  need = _bound(code, dev.rows, 2, 1)[2]
  buf = np.zeros((need + 32,), np.uint8)
  base = (rn.ptr(buf) + 15) // 16 * 16
  dev.ws, dev.ws_bytes = base, need - 1
  _refused(dev, rn.RA_E_WORKSPACE, 'ws_bytes=%d' % (need - 1), '%d bytes' % need)
  dev.ws, dev.ws_bytes = base + 4, need
  _refused(dev, rn.RA_E_WORKSPACE, '16-byte boundary')
  # the bound queries
  assert _bound(code, [(0, 2, 5)], 1, 2)[0] == rn.RA_E_SHAPE and 'bpp=2' in rn.lib().ra_last_error_string().decode()
  assert _bound(code, [(0, 2, 5), (10, 0, 1)], 1, 1)[0] == rn.RA_E_SHAPE and 'image 1' in rn.lib().ra_last_error_string().decode()


def test_the_wrappers_refuse_what_they_can_see():
  src, geo, _ = rc.layout('mixed', 'grey', 'packed')
  with pytest.raises(rn.RecAttendError, match='plane_index'):
    ops.png_deflate_ragged_host(src, geo, [len(src)])
  with pytest.raises(rn.RecAttendError, match="code='huffman'"):
    ops.png_deflate_ragged_host(src, geo, code='huffman')
  with pytest.raises(rn.RecAttendError, match='src must be'):
    ops.png_deflate_ragged_host(src.astype(np.int32), geo)
  with pytest.raises(rn.RecAttendError, match='on the device'):
    ops.png_deflate_ragged(torch.from_numpy(src), geo)
  with pytest.raises(rn.RecAttendError, match='image 7'):  # the flat buffer is a byte short of the table
    ops.png_deflate_ragged_host(src[:, :-1], geo)


def test_ragged_picture_is_the_list_of_views_it_replaces():
  import analysis
  geo, total = ops.ragged_geometry([(3, 5), (2, 7), (4, 1)], 4)
  flat = torch.arange(total * 3, dtype=torch.int64).remainder(251).to(torch.uint8).view(total, 3)
  pic = analysis.RaggedPicture(flat, geo)
  views = [flat[o:o + h * w].view(h, w, 3) for o, h, w in geo.tolist()]
  assert len(pic) == 3 and pic.flat is flat and np.array_equal(pic.geo, geo)
  for got, want in zip(pic, views):
    assert got.shape == want.shape and torch.equal(got, want) and got.data_ptr() == want.data_ptr()  # views that alias flat
  assert [tuple(p.shape) for p in pic] == [(3, 5, 3), (2, 7, 3), (4, 1, 3)]
  assert torch.equal(pic[-1], views[2]) and [v.data_ptr() for v in pic[1:]] == [v.data_ptr() for v in views[1:]]
  pic[1][0, 0, 0] = 255
  assert int(flat[geo[1, 0], 0]) == 255
  with pytest.raises(IndexError):
    pic[3]
  with pytest.raises(rn.RecAttendError, match='RaggedPicture'):
    analysis.RaggedPicture(flat.view(-1), geo)


def test_render_analyzer_takes_a_ragged_picture_on_the_host_route(tmp_path):
  """Without device_png a RaggedPicture is written as the list it replaces: the host writer, image by image."""
  import analysis
  from utils import png
  geo, total = ops.ragged_geometry([(3, 5), (2, 7)], 4)
  flat = torch.arange(total * 3, dtype=torch.int64).remainder(251).to(torch.uint8).view(total, 3)
  an = analysis.RenderInstanceAnalyzer(str(tmp_path), ['a.png', 'b.png'])
  an.stage({'picture': analysis.RaggedPicture(flat, geo), 'indices': [0, 1]})
  for name, (o, h, w) in zip('ab', geo.tolist()):
    assert np.array_equal(png.read_colour8(str(tmp_path / (name + '.png'))), flat[o:o + h * w].view(h, w, 3).numpy())
