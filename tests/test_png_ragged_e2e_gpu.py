"""The ragged PNG encoder behind the two command lines that write batches of mixed sizes, on the MI355X:
full_model_eval.py --render_from_ids --render_gt_from_ids --device_png (analysis.RaggedPicture -> ONE write_colour8_ragged_dev call
per written batch) and fg_model_eval.py --device_png on a mixed archive (the thresholded planes of a batch in one flat buffer ->
ONE write_gray8_ragged_dev call, gt/ one more).  The files are those of the run without the flag — same names, same decoded
pixels — their IDAT payload is the uniform host entry's stream of that picture alone, and count.csv does not change.  The
archives are the smallest ones of tests/test_ins_render_e2e_gpu.py and tests/test_ragged_e2e_gpu.py, restated."""
import os

import numpy as np
import pytest
import yaml

import ra_ops as ops
import ra_oracle as ora
import setup_labels
from utils import png

pytestmark = pytest.mark.gpu
SIZES = ((96, 80), (90, 84), (100, 72))
NAMES = ['a.png', 'b.png', 'c.png']
FOLDERS = ('30', '50')


class _Calls(object):
  """Counts the calls of the two device encoders' wrappers while the command line runs."""

  def __init__(self, monkeypatch):
    self.ragged, self.uniform = [], []
    ragged, uniform = ops.png_deflate_ragged, ops.png_deflate

    def count_ragged(src, geo, *a, **k):
      self.ragged.append((tuple(src.shape), len(geo)))
      return ragged(src, geo, *a, **k)

    def count_uniform(src, *a, **k):
      self.uniform.append(tuple(src.shape))
      return uniform(src, *a, **k)
    monkeypatch.setattr(ops, 'png_deflate_ragged', count_ragged)
    monkeypatch.setattr(ops, 'png_deflate', count_uniform)


def _idat(path):
  with open(path, 'rb') as f:
    return b''.join(payload for tag, payload, _ in png.iter_chunks(f.read()) if tag == b'IDAT')


def _discs(rng, h, w):
  rr, cc = np.mgrid[0:h, 0:w]
  img = np.zeros((h, w), np.int32)
  for i in range(3):
    cy, cx, rad = rng.uniform(10, h - 10), rng.uniform(10, w - 10), rng.uniform(8, 20)
    img[(rr - cy) ** 2 + (cc - cx) ** 2 <= rad ** 2] = i + 1
  return img


def test_full_model_eval_writes_a_mixed_batch_in_one_call(cuda, tmp_path, monkeypatch):
  import full_model_eval
  opt = ora.make_opt('cvppp', 64, 64, 2)  # the shapes of smoke()
  res = str(tmp_path / 'results')
  os.makedirs(os.path.join(res, 'm0'))
  with open(os.path.join(res, 'm0', 'model_opt.yaml'), 'w') as f:
    yaml.safe_dump(opt, f)
  np.savez(os.path.join(res, 'm0', 'weights.npz'), **ora.random_params(opt, 1))
  rng = np.random.RandomState(2)
  x = rng.rand(len(SIZES), 64, 64, 3).astype(np.float32)
  imgs = [_discs(rng, h, w) for h, w in SIZES]
  path = str(tmp_path / 'mixed.npz')
  np.savez(path, x=x, names=np.array(NAMES), **setup_labels.flatten_images(imgs))

  def run(tag, *flags):
    out = str(tmp_path / ('out_' + tag))
    full_model_eval.main(['--model_id', 'm0', '--results', res, '--input', path, '--output', out, '--batch_size', '2',
                          '--threshold_list', '0.3,0.5', '--render_from_ids', '--render_gt_from_ids'] + list(flags))
    return os.path.join(out, 'output_valid')

  host = run('host')
  keys = [(sub, n) for sub in FOLDERS + ('gt',) for n in NAMES]
  want = {k: png.read_colour8(os.path.join(host, *k)) for k in keys}
  assert any((want[('30', n)] != 0).any() for n in NAMES) and any((want[('gt', n)] != 0).any() for n in NAMES)
  for code in ('fixed', 'dynamic'):
    calls = _Calls(monkeypatch)
    dev = run(code, '--device_png', '--device_png_code', code)
    monkeypatch.undo()
    # batches of 2 and 1 images; per batch one call per threshold and one for gt/: whatever the sizes, never one per size
    assert calls.uniform == []
    assert sorted(b for _, b in calls.ragged) == [1, 1, 1, 2, 2, 2] and all(len(s) == 2 and s[1] == 3 for s, _ in calls.ragged)
    for k, (h, w) in zip(keys, SIZES * 3):
      file = os.path.join(dev, *k)
      got = png.read_colour8(file)
      assert got.shape == (h, w, 3) and np.array_equal(got, want[k]), (code, k)
      assert _idat(file) == ops.png_deflate_host(want[k][None], code=code)[0][0], (code, k)
    for sub in FOLDERS:
      with open(os.path.join(dev, sub, 'count.csv')) as f, open(os.path.join(host, sub, 'count.csv')) as g:
        assert f.read() == g.read()
    assert sorted(os.listdir(os.path.join(dev, 'gt'))) == sorted(os.listdir(os.path.join(host, 'gt'))) == sorted(NAMES)


def test_fg_model_eval_writes_a_mixed_batch_in_one_call(cuda, tmp_path, monkeypatch):
  import fg_eval_oracle as feo
  import fg_model_eval
  import fg_oracle as fo
  opt = dict(fo.reduced_opt(1, True), segm_loss_fn='bce')
  res = str(tmp_path / 'results')
  os.makedirs(os.path.join(res, 'fg'))
  with open(os.path.join(res, 'fg', 'model_opt.yaml'), 'w') as f:
    yaml.safe_dump(opt, f)
  np.savez(os.path.join(res, 'fg', 'weights.npz'), step=np.float32(1), **fo.random_weights(opt, 71))
  rng = np.random.RandomState(73)
  x = rng.rand(3, 32, 48, 3).astype(np.float32)
  gts = [feo.disc_labels(rng, 1, h, w)[0] for h, w in SIZES]
  offset = np.zeros(4, np.int64)
  for i, g in enumerate(gts):
    offset[i + 1] = -(-(offset[i] + g.size) // 4) * 4
  flat = np.zeros(int(offset[-1]), np.uint8)
  for i, g in enumerate(gts):
    flat[offset[i]:offset[i] + g.size] = g.reshape(-1)
  path = str(tmp_path / 'mixed.npz')
  np.savez(path, x=x, names=np.array(NAMES), fg_gt_full_flat=flat, pixel_offset=offset, orig_size=np.array(SIZES, np.int32))

  def run(tag, *flags):
    out = str(tmp_path / ('out_' + tag))
    fg_model_eval.main(['--model_id', 'fg', '--results', res, '--input', path, '--output', out, '--batch_size', '2', '--threshold_list',
                        '0.3,0.5', '--render_gt', '--render_soft'] + list(flags))
    return out

  host = run('host')
  keys = [(sub, n) for sub in FOLDERS + ('gt', 'soft') for n in NAMES]
  want = {k: png.read_gray8(os.path.join(host, *k)) for k in keys}
  assert any(want[('30', n)].any() for n in NAMES) and any(want[('gt', n)].any() for n in NAMES)
  for code in ('fixed', 'dynamic'):
    calls = _Calls(monkeypatch)
    dev = run(code, '--device_png', '--device_png_code', code)
    monkeypatch.undo()
    # batches of 2 and 1 images: ONE call for both thresholds and one for gt/ per batch
    assert calls.uniform == []
    assert sorted(calls.ragged) == sorted([((2, int(offset[2])), 2), ((int(offset[2]),), 2), ((2, int(offset[3] - offset[2])), 1),
                                           ((int(offset[3] - offset[2]),), 1)])
    for k, (h, w) in zip(keys, SIZES * 4):
      file = os.path.join(dev, *k)
      got = png.read_gray8(file)
      assert got.shape == (h, w) and np.array_equal(got, want[k]), (code, k)
      if k[0] != 'soft':  # soft/ stays with the host's zlib
        assert _idat(file) == ops.png_deflate_host(want[k][None], code=code)[0][0], (code, k)
    with open(os.path.join(dev, 'metrics.yaml')) as f, open(os.path.join(host, 'metrics.yaml')) as g:
      assert yaml.safe_load(f) == yaml.safe_load(g)
