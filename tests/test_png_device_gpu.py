"""The device PNG encoder on the MI355X (csrc/ra_png.hip): its streams against ra_png_deflate_host byte for byte on the case list
of tests/test_png_device.py (where the host entry is held against zlib and the Python restatement), batches, unaligned sources,
the float source with a plane list, one real-size image, and the three command lines with and without --device_png."""
import os
import zlib

import numpy as np
import pytest
import torch

import png_cases as pc
import ra_ops as ops
from utils import png

pytestmark = pytest.mark.gpu


def _raw(img):
  img = np.asarray(img)
  rows = (img[:, :, ::-1] if img.ndim == 3 else img).reshape(img.shape[0], -1)
  return np.concatenate([np.zeros((img.shape[0], 1), np.uint8), rows], axis=1).tobytes()


def _device_equals_host(batch, plane_index=None):
  """batch: a NumPy array of one of the three source kinds; returns the streams."""
  want, adler = ops.png_deflate_host(batch, plane_index)
  got, sizes, offsets, dev_adler = ops.png_deflate(torch.from_numpy(batch).cuda(), plane_index, with_meta=True)
  assert len(got) == len(want)
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


@pytest.mark.parametrize('kind', pc.KINDS)
def test_batch_of_different_images(cuda, kind):
  """N = 5 images of 40 x 300 in one call: the streams lie back to back, each decodes to its own image."""
  rs = np.random.RandomState(17)
  shape = (40, 300) if kind == 'grey' else (40, 300, 3)
  imgs = [np.zeros(shape, np.uint8), rs.randint(0, 256, size=shape).astype(np.uint8), pc.alternating(kind, 40, 300),
          (rs.rand(*shape) > 0.97).astype(np.uint8) * 255, np.full(shape, 255, np.uint8)]
  got = _device_equals_host(np.stack(imgs))
  assert len(set(got)) == 5
  for img, z in zip(imgs, got):
    assert zlib.decompress(z) == _raw(img)


@pytest.mark.parametrize('kind', pc.KINDS)
def test_unaligned_sources_take_the_element_loads(cuda, kind):
  """A width that is a multiple of 16 (the 16-byte form) read from a base that is not 16-byte aligned, and an odd H * W: the
  same bytes as the host gives."""
  rs = np.random.RandomState(23)
  c = () if kind == 'grey' else (3,)
  whole = (rs.rand(3, 9, 64, *c) > 0.8).astype(np.uint8) * 255
  flat = torch.from_numpy(whole).cuda().reshape(-1)
  per = whole[0].size
  for shift in (1, 4, 8):  # a sliced source: two images from `shift` bytes into the buffer
    view = flat[shift:shift + 2 * per].view(2, *whole.shape[1:])
    assert view.data_ptr() % 16 == shift and view.is_contiguous()
    want, _ = ops.png_deflate_host(whole.reshape(-1)[shift:shift + 2 * per].reshape(2, *whole.shape[1:]))
    assert ops.png_deflate(view) == want
  assert ops.png_deflate(flat[:2 * per].view(2, *whole.shape[1:])) == ops.png_deflate_host(whole[:2])[0]  # the aligned twin
  odd = (rs.rand(3, 7, 33, *c) > 0.5).astype(np.uint8) * 255  # odd H * W: the second image starts at an odd address
  _device_equals_host(odd)


def test_float_source_with_a_plane_list(cuda):
  ks = np.arange(256, dtype=np.float32) / np.float32(255.0)
  for W in (70, 64):  # element loads / 16-byte loads
    y = np.zeros((6, 5, W), np.float32)
    y[0], y[1], y[3] = 1.0, 0.5, 0.999
    y[2] = np.resize(ks, (5, W))
    y[4] = np.random.RandomState(3).rand(5, W) > 0.5
    y[5] = np.resize(ks[::-1], (5, W))
    dev = torch.from_numpy(y).cuda()
    want = (dev * 255).to(torch.uint8).cpu().numpy()  # the analyzer's own expression
    assert np.array_equal(want, (y * np.float32(255.0)).astype(np.uint8)) and want[3, 0, 0] == 254 and want[1, 0, 0] == 127
    planes = [5, 0, 0, 3, 1, 2]  # skips 4, repeats 0, out of order
    got = _device_equals_host(y, planes)
    for p, z in zip(planes, got):
      assert zlib.decompress(z) == _raw(want[p])
    assert [zlib.decompress(z) for z in ops.png_deflate(dev)] == [_raw(w) for w in want]
    assert [zlib.decompress(z) for z in ops.png_deflate(dev[1:], [3, 3])] == [_raw(want[4])] * 2  # a view at an offset


def test_one_real_size_colour_image(cuda):
  """1024 x 2048, T = 20 flat-colour discs: 1024 workgroups of 6145-byte segments; decoded with zlib and compared."""
  yy, xx = torch.meshgrid(torch.arange(1024, device='cuda'), torch.arange(2048, device='cuda'), indexing='ij')
  img = torch.zeros((1, 1024, 2048, 3), dtype=torch.uint8, device='cuda')
  rs = np.random.RandomState(5)
  for t in range(20):
    cy, cx, r = rs.randint(100, 924), rs.randint(100, 1948), rs.randint(40, 160)
    img[0][(yy - cy) ** 2 + (xx - cx) ** 2 < r * r] = torch.tensor(rs.randint(1, 256, size=3).astype(np.uint8), device='cuda')
  files = png.encode_colour8_dev(img)
  host = img[0].cpu().numpy()
  z = b''.join(payload for tag, payload, _ in png.iter_chunks(files[0]) if tag == b'IDAT')
  assert zlib.decompress(z) == _raw(host)
  assert np.array_equal(png.decode_colour8(files[0]), host)
  assert len(z) < ops.png_deflate_bound(1, 1024, 2048, 3)[0] // 20  # flat colours: far below the bound
  mask = (img[:, :, :, 0] > 0).to(torch.uint8) * 255
  assert np.array_equal(png.decode_gray8(png.encode_gray8_dev(mask)[0]), mask[0].cpu().numpy())


def test_capacity_is_checked_on_the_host(cuda):
  """A capacity one byte below the bound is refused by name, nothing is launched and nothing written."""
  import ra_native as rn
  src = torch.zeros((2, 4, 16), dtype=torch.uint8, device='cuda')
  stream, ws_bytes = ops.png_deflate_bound(2, 4, 16, 1)
  out = torch.full((2 * stream,), 0xAB, dtype=torch.uint8, device='cuda')
  ws = torch.empty((ws_bytes,), dtype=torch.uint8, device='cuda')
  meta = torch.full((8,), -7, dtype=torch.int32, device='cuda')
  rc = rn.lib().ra_png_deflate_u8(rn.ptr(src), rn.RA_PNG_GRAY8, 2, 2, 4, 16, None, rn.ptr(out), 2 * stream - 1, rn.ptr(meta[:2]),
                                  rn.ptr(meta[4:]), rn.ptr(meta[2:4]), rn.ptr(ws), ws_bytes, rn.stream_ptr())
  assert rc == rn.RA_E_WORKSPACE and 'out_bytes' in rn.lib().ra_last_error_string().decode()
  torch.cuda.synchronize()
  assert bool((out == 0xAB).all()) and bool((meta == -7).all())


# ---- the command lines: the same files, the same text, the same pixels
def _tree(root):
  out = {}
  for base, _, files in os.walk(root):
    for f in files:
      out[os.path.relpath(os.path.join(base, f), root)] = os.path.join(base, f)
  return out


def _same_outputs(a, b, identical=()):
  """Folder b (--device_png) against folder a: the same file names; every text file (.txt, .csv, .yaml, .json) byte-identical;
  every PNG decoding to its twin's pixels — and differing in its bytes, unless its folder is listed in `identical`."""
  ta, tb = _tree(a), _tree(b)
  assert sorted(ta) == sorted(tb)
  n_png = 0
  for rel in sorted(ta):
    if rel.endswith('.npz'):  # a zip archive carries the time it was written
      continue
    da, db = open(ta[rel], 'rb').read(), open(tb[rel], 'rb').read()
    if not rel.endswith('.png') or rel.split(os.sep)[0] in identical or os.path.basename(os.path.dirname(rel)) in identical:
      assert da == db, rel
      continue
    assert np.array_equal(png.decode_colour8(da), png.decode_colour8(db)), rel
    assert da != db, rel  # the flag did take the other encoder
    n_png += 1
  return n_png


def test_cityscapes_eval_device_png(cuda, tmp_path):
  import cityscapes_eval as ce
  import cs_oracle as co
  scenes = [co.synthetic_scene(sd) for sd in (11, 12, 13)]
  names = ['aachen_000001_000019.png', 'aachen_000002_000019.png', 'bochum_000001_000019']
  y, s, sem = (np.concatenate([sc[k] for sc in scenes]) for k in range(3))
  gt = (co.resize_linear(y, 128, 256) > 0.5).astype(np.float32)
  src = str(tmp_path / 'in.npz')
  np.savez(src, y_out_ins=y, s_out=s, y_out=sem, y_gt_full=gt, s_gt=np.ones(s.shape, np.float32), names=np.array(names))
  common = ['--input', src, '--threshold_list', '0.3,0.5', '--remove_tiny', '120', '--batch_size', '2', '--analyzers', 'sbd',
            '--render_instances']
  a, b = str(tmp_path / 'host'), str(tmp_path / 'dev')
  ce.main(common + ['--output', a])
  ce.main(common + ['--output', b, '--device_png'])
  assert _same_outputs(a, b) >= 6 + 3 * 3  # the masks, and three images in each of 30/, 50/ and gt/


def test_full_model_eval_render_device_png(cuda, tmp_path):
  import full_model_eval
  import full_model_train
  from test_loss_gpu import synth_gt
  res = str(tmp_path / 'results')
  full_model_train.main(['--init_only', '--results', res, '--model_id', 'm0', '--inp_height', '64',
                         '--inp_width', '64', '--timespan', '4', '--ctrl_add_inp', '--ctrl_add_canvas',
                         '--attn_add_inp', '--attn_add_canvas', '--fixed_gamma',
                         '--ctrl_cnn_filter_size', '3,3,3,3', '--ctrl_cnn_depth', '8,8,16,16',
                         '--ctrl_cnn_pool', '1,2,1,2', '--attn_cnn_filter_size', '3,3,3,3,3,3',
                         '--attn_cnn_depth', '8,8,16,16,32,32', '--attn_cnn_pool', '1,2,1,2,1,2',
                         '--attn_dcnn_filter_size', '3,3,3,3,3,3,3', '--attn_dcnn_depth', '32,32,16,16,8,8,1',
                         '--attn_dcnn_pool', '2,1,2,1,2,1,1'])
  rng = np.random.RandomState(4)
  x = rng.rand(3, 64, 64, 3).astype(np.float32)
  y_gt, s_gt = synth_gt(rng, 3, 4, 64, 64, max_inst=3)
  inp = str(tmp_path / 'in.npz')
  np.savez(inp, x=x, y_gt=y_gt, s_gt=s_gt, names=np.array(['img_a.png', 'img_b.png', 'img_c.png']))
  common = ['--model_id', 'm0', '--results', res, '--input', inp, '--batch_size', '2', '--threshold_list', '0.3,0.55',
            '--analyzers', 'sbd', '--render', '--render_gt_instances']
  a, b = str(tmp_path / 'host'), str(tmp_path / 'dev')
  full_model_eval.main(common + ['--output', a])
  full_model_eval.main(common + ['--output', b, '--device_png'])
  assert _same_outputs(a, b) == 9


def test_fg_model_eval_device_png(cuda, tmp_path):
  import yaml
  import fg_eval_oracle as feo
  import fg_model_eval
  import fg_oracle as fo
  opt = dict(fo.reduced_opt(1, True), segm_loss_fn='bce')
  res = str(tmp_path / 'results')
  os.makedirs(os.path.join(res, 'fg'))
  with open(os.path.join(res, 'fg', 'model_opt.yaml'), 'w') as f:
    yaml.safe_dump(opt, f)
  np.savez(os.path.join(res, 'fg', 'weights.npz'), step=np.float32(1), **fo.random_weights(opt, 61))
  rng = np.random.RandomState(62)
  N, h, w, H, W = 3, 32, 48, 61, 103
  src = str(tmp_path / 'in.npz')
  np.savez(src, x=rng.rand(N, h, w, 3).astype(np.float32), fg_gt_full=feo.disc_labels(rng, N, H, W), names=np.array(['a.png', 'b.png', 'c.png']))
  common = ['--model_id', 'fg', '--results', res, '--input', src, '--batch_size', '2', '--threshold_list', '0.5,0.45',
            '--render_soft', '--render_gt', '--render_orientation']
  a, b = str(tmp_path / 'host'), str(tmp_path / 'dev')
  fg_model_eval.main(common + ['--output', a])
  fg_model_eval.main(common + ['--output', b, '--device_png'])
  assert _same_outputs(a, b, identical=('soft',)) == 3 * 4  # 45/, 50/, gt/ and ori/; soft/ stays with the host's zlib
