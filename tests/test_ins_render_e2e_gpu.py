"""full_model_eval.py --render_from_ids --render_gt_from_ids end to end on the MI355X: a uniform archive of id images, a mixed
archive of three sizes (with and without a foreground + --remove_tiny), the same through --device_png in both stream formats,
and a flat archive of one size against the uniform one.  Every file decodes to its image's own size, the mixed run's pictures
are the one-image runs' pictures, every palette colour covers exactly the area the counting pass counted for that prediction
(from the run's own pred_rank0.npz, through ops.instance_eval_counts WITHOUT the map), and count.csv agrees with the yaml's
counting analyzers.  The model and the archives are the ones tests/test_ragged_e2e_gpu.py builds its inputs from, restated."""
import os

import numpy as np
import pytest
import torch
import yaml

import ins_render_oracle as iro
import ra_ops as ops
import ra_oracle as ora
import setup_labels
from utils import png

pytestmark = pytest.mark.gpu
SIZES = ((96, 80), (90, 84), (100, 72))
NAMES = ['a.png', 'b.png', 'c.png']
THRESHOLDS = (0.3, 0.5)
FOLDERS = ('30', '50')
TINY = 60


def _model(tmp_path):
  opt = ora.make_opt('cvppp', 64, 64, 2)  # the shapes of smoke()
  res = str(tmp_path / 'results')
  os.makedirs(os.path.join(res, 'm0'))
  with open(os.path.join(res, 'm0', 'model_opt.yaml'), 'w') as f:
    yaml.safe_dump(opt, f)
  np.savez(os.path.join(res, 'm0', 'weights.npz'), **ora.random_params(opt, 1))
  return res


def _discs(rng, h, w):
  rr, cc = np.mgrid[0:h, 0:w]
  img = np.zeros((h, w), np.int32)
  for i in range(3):
    cy, cx, rad = rng.uniform(10, h - 10), rng.uniform(10, w - 10), rng.uniform(8, 20)
    img[(rr - cy) ** 2 + (cc - cx) ** 2 <= rad ** 2] = i + 1
  return img


def _mixed_inputs(seed=2):
  rng = np.random.RandomState(seed)
  x = rng.rand(len(SIZES), 64, 64, 3).astype(np.float32)
  return x, [_discs(rng, h, w) for h, w in SIZES]


def _uniform_inputs(seed=2):
  rng = np.random.RandomState(seed)
  x = rng.rand(3, 64, 64, 3).astype(np.float32)
  return x, np.stack([_discs(rng, 96, 80) for _ in range(3)])


def _ellipse(h, w, n):
  rr, cc = np.mgrid[0:h, 0:w]
  return ((rr - h / 2.0) ** 2 / (0.42 * h) ** 2 + (cc - w / 2.0 - 6 * n) ** 2 / (0.38 * w) ** 2 <= 1).astype(np.uint8)


def _run(tmp_path, res, tag, *flags, **arrays):
  import full_model_eval
  path, out = str(tmp_path / (tag + '.npz')), str(tmp_path / ('out_' + tag))
  np.savez(path, **arrays)
  full_model_eval.main(['--model_id', 'm0', '--results', res, '--input', path, '--output', out, '--batch_size', '2', '--threshold_list',
                        '0.3,0.5', '--render_from_ids', '--render_gt_from_ids'] + list(flags))
  return os.path.join(out, 'output_valid')


def _pictures(folder, names=NAMES):
  """{(subfolder, name): uint8 [h,w,3]} of every file the two flags write."""
  return {(sub, n): png.read_colour8(os.path.join(folder, sub, n)) for sub in FOLDERS + ('gt',) for n in names}


def _check_run(folder, ids_list, fgs=None, tiny=0, names=NAMES):
  """Sizes, areas per palette colour and count.csv of one run against its own pred_rank0.npz and metrics_rank0.yaml."""
  pics = _pictures(folder, names)
  pred = np.load(os.path.join(folder, 'pred_rank0.npz'))
  with open(os.path.join(folder, 'metrics_rank0.yaml')) as f:
    met = yaml.safe_load(f)
  tab = iro.default_colours(2)
  counted = {sub: [] for sub in FOLDERS}
  for i, (name, ids) in enumerate(zip(names, ids_list)):
    for sub in FOLDERS + ('gt',):
      assert pics[(sub, name)].shape == ids.shape + (3,), (sub, name)
    yc = torch.from_numpy(pred['y_out'][i:i + 1] * pred['s_out'][i:i + 1, :, None, None]).cuda()
    conf = torch.from_numpy((pred['s_out'][i:i + 1] > 0.5).astype(np.float32)).cuda()
    gt = torch.from_numpy(ids[None].astype(np.int32)).cuda()
    lab = ops.assemble_labels(ids[None], 64, 64, 2, 'cvppp', want=('inst_id', 's_gt'))
    fg = None if fgs is None else torch.from_numpy(fgs[i][None]).cuda()
    inter, area_b = ops.instance_eval_counts(yc, gt, lab['inst_id'], list(THRESHOLDS), fg=fg, morph=fg is not None)
    per = ops.eval_metrics_from_counts(inter, area_b, lab['s_gt'], remove_tiny=tiny if fg is not None else 0, conf=conf)
    for sub, m in zip(FOLDERS, per):
      sizes = m['sizes'][0].cpu().numpy()
      img = pics[(sub, name)]
      for t in range(2):
        assert int((img == tab[t]).all(axis=-1).sum()) == int(sizes[t]), (sub, name, t)
      assert int((img != 0).any(axis=-1).sum()) == int(sizes.sum())
      counted[sub].append((int((sizes > 0).sum()), int(lab['s_gt'][0].sum())))
    # the ground truth: every pixel of a listed instance has a colour, the rest is black
    listed = np.isin(ids, lab['inst_id'][0].cpu().numpy()[lab['inst_id'][0].cpu().numpy() >= 0])
    assert (((pics[('gt', name)] != 0).any(axis=-1)) == listed).all(), name
  for sub, th in zip(FOLDERS, ('0.30', '0.50')):
    with open(os.path.join(folder, sub, 'count.csv')) as f:
      rows = [line.strip().split(',') for line in f]
    assert rows[0] == ['Image ID', 'Count Out', 'Count GT']
    assert sorted((int(r[0]), int(r[1]), int(r[2])) for r in rows[1:]) == [(i,) + c for i, c in enumerate(counted[sub])]
    d = np.array([c[0] - c[1] for c in counted[sub]], np.float64)
    assert met[th]['dic']['mean'] == pytest.approx(d.mean(), abs=1e-6) and met[th]['dic_abs']['mean'] == pytest.approx(np.abs(d).mean(), abs=1e-6)
    assert met[th]['count_acc']['mean'] == pytest.approx((d == 0).mean(), abs=1e-6) and met[th]['dic']['count'] == len(names)
  return pics


def test_uniform_archive_and_its_flat_twin(cuda, tmp_path):
  res = _model(tmp_path)
  x, ids = _uniform_inputs()
  folder = _run(tmp_path, res, 'uniform', x=x, names=np.array(NAMES), gt_instance_ids=ids)
  pics = _check_run(folder, list(ids))
  assert any((pics[('30', n)] != 0).any() for n in NAMES) and any((pics[('gt', n)] != 0).any() for n in NAMES)
  flat = _run(tmp_path, res, 'uniform_flat', x=x, names=np.array(NAMES), **setup_labels.flatten_images(list(ids)))
  twin = _pictures(flat)
  for key in pics:
    assert np.array_equal(pics[key], twin[key]), key
  with open(os.path.join(folder, 'metrics_rank0.yaml')) as f, open(os.path.join(flat, 'metrics_rank0.yaml')) as g:
    assert yaml.safe_load(f) == yaml.safe_load(g)


@pytest.mark.parametrize('with_fg', [False, True])
def test_mixed_archive_against_one_image_runs(cuda, tmp_path, with_fg):
  res = _model(tmp_path)
  x, imgs = _mixed_inputs()
  fgs = [_ellipse(h, w, n) for n, (h, w) in enumerate(SIZES)] if with_fg else None
  flags = ['--remove_tiny', str(TINY)] if with_fg else []
  flat = setup_labels.flatten_images(imgs)
  extra = {}
  if with_fg:
    fg_flat = np.zeros(flat['gt_instance_ids_flat'].shape, np.uint8)
    for i, f in enumerate(fgs):
      o = int(flat['pixel_offset'][i])
      fg_flat[o:o + f.size] = f.reshape(-1)
    extra['fg_flat'] = fg_flat
  folder = _run(tmp_path, res, 'mixed', *flags, x=x, names=np.array(NAMES), **dict(flat, **extra))
  pics = _check_run(folder, imgs, fgs, TINY)
  assert any((pics[('30', n)] != 0).any() for n in NAMES)
  for i, name in enumerate(NAMES):
    one = dict(fg=fgs[i][None]) if with_fg else {}
    single = _pictures(_run(tmp_path, res, 'one%d' % i, *flags, x=x[i:i + 1], names=np.array([name]), gt_instance_ids=imgs[i][None], **one),
                       [name])
    for key in single:
      assert np.array_equal(single[key], pics[key]), key


def test_device_png_gives_the_same_pixels(cuda, tmp_path):
  res = _model(tmp_path)
  x, imgs = _mixed_inputs()
  arrays = dict(x=x, names=np.array(NAMES), **setup_labels.flatten_images(imgs))
  host = _pictures(_run(tmp_path, res, 'host', **arrays))
  for tag, flags in (('fixed', ['--device_png']), ('dynamic', ['--device_png', '--device_png_code', 'dynamic'])):
    dev = _pictures(_run(tmp_path, res, tag, *flags, **arrays))
    for key in host:
      assert np.array_equal(host[key], dev[key]), (tag, key)
  x1, ids = _uniform_inputs()
  arrays = dict(x=x1, names=np.array(NAMES), gt_instance_ids=ids)
  host = _pictures(_run(tmp_path, res, 'uhost', **arrays))
  dev = _pictures(_run(tmp_path, res, 'udev', '--device_png', **arrays))
  for key in host:
    assert np.array_equal(host[key], dev[key]), key
