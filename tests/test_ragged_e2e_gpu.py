"""Mixed full sizes end to end on the MI355X: setup_labels.py --mixed_sizes on a folder of three sizes, full_model_eval.py
and fg_model_eval.py on archives in the flat format against one-image archives through the paths that existed before, the
trainers' label assembly from a flat archive, and one refusal by name per refused flag."""
import os

import numpy as np
import pytest
import torch
import yaml

import ins_eval_oracle as ieo
import labels_oracle as lo
import ra_native as rn
import ra_ops as ops
import setup_labels
from test_ins_eval_gpu import _e2e_inputs, _e2e_model
from utils import png

pytestmark = pytest.mark.gpu
SIZES = ((96, 80), (90, 84), (100, 72))
NAMES = ['a.png', 'b.png', 'c.png']
E2E_SEED = 2  # the first seed tried; the band it gives is asserted below


def _id_images(seed=E2E_SEED):
  """x [3,64,64,3] and one id image per size: three discs each, as tests/test_ins_eval_gpu.py::_e2e_inputs paints them."""
  rng = np.random.RandomState(seed)
  x = rng.rand(len(SIZES), 64, 64, 3).astype(np.float32)
  imgs = []
  for h, w in SIZES:
    rr, cc = np.mgrid[0:h, 0:w]
    img = np.zeros((h, w), np.int32)
    for i in range(3):
      cy, cx, rad = rng.uniform(10, h - 10), rng.uniform(10, w - 10), rng.uniform(8, 20)
      img[(rr - cy) ** 2 + (cc - cx) ** 2 <= rad ** 2] = i + 1
    imgs.append(img)
  return x, imgs


def test_full_model_eval_on_mixed_sizes(cuda, tmp_path, monkeypatch):
  import full_model
  import full_model_eval
  res, opt = _e2e_model(tmp_path)
  x, imgs = _id_images()
  thresholds = [0.3, 0.5]
  # the condition on the inputs, which needs the device: per image an empty band and no ties for what this model decodes
  model = full_model.get_model(dict(opt, use_knob=False)).load_weights(dict(np.load(os.path.join(res, 'm0', 'weights.npz'))))
  y_out, s_out = model.run(['y_out', 's_out'], {'x': x, 'phase_train': False}, as_numpy=True)
  yc = (torch.from_numpy(y_out) * torch.from_numpy(s_out)[:, :, None, None]).numpy()
  for i, img in enumerate(imgs):
    inst_id = ops.assemble_labels(img[None], 64, 64, 2, 'cvppp', want=('inst_id',))['inst_id'].cpu().numpy()
    lo_, hi_, share, ties = ieo.conditions(ieo.values(yc[i:i + 1], img.shape[0], img.shape[1], False), img[None], inst_id, thresholds, None)
    print('image %d %s: undecided share %.5f, band of %d counts, exact ties %d' % (i, img.shape, share, int((hi_ - lo_).sum()), ties))
    assert (lo_ == hi_).all() and ties == 0

  def run(tag, *flags, **arrays):
    path, out = str(tmp_path / (tag + '.npz')), str(tmp_path / ('out_' + tag))
    np.savez(path, **arrays)
    full_model_eval.main(['--model_id', 'm0', '--results', res, '--input', path, '--output', out, '--batch_size', '2',
                          '--threshold_list', '0.3,0.5'] + list(flags))
    with open(os.path.join(out, 'output_valid', 'metrics_rank0.yaml')) as f:
      return yaml.safe_load(f)

  flat = setup_labels.flatten_images(imgs)
  assert len({tuple(s) for s in flat['orig_size'].tolist()}) == 3
  got = run('mixed', x=x, names=np.array(NAMES), **flat)
  # The one-image runs, with every analyzer's values recorded as they are staged: metrics_rank0.yaml holds the mean that
  # NumPy forms over the concatenated float32 values, so the mean the three images must give is formed from their values in
  # the same way (a mean of the three yaml means would be another float32 rounding away, not 1e-12).
  import analysis
  staged, create = [], analysis.create_analyzer

  def recording(n):
    a = create(n)

    def call(results):
      v = a(results)
      staged[-1].setdefault(n, []).append(v.cpu().numpy())  # one entry per threshold: a one-image run is one batch
      return v
    return call

  singles = []
  monkeypatch.setattr(analysis, 'create_analyzer', recording)
  for i in range(3):
    staged.append({})
    singles.append(run('one%d' % i, x=x[i:i + 1], names=np.array(NAMES[i:i + 1]), gt_instance_ids=imgs[i][None]))
  monkeypatch.undo()
  assert sorted(got) == ['0.30', '0.50']
  for k, th in enumerate(sorted(got)):
    assert sorted(got[th]) == sorted(singles[0][th])
    for n in got[th]:  # analyzer by analyzer: the counts equal, the means to 1e-12
      vals = np.concatenate([st[n][k] for st in staged])
      for s, st in zip(singles, staged):  # the recorder saw what the yaml of the one-image run holds
        assert s[th][n]['count'] == st[n][k].size and (st[n][k].size == 0 or s[th][n]['mean'] == float(st[n][k].mean()))
      assert got[th][n]['count'] == vals.size == sum(s[th][n]['count'] for s in singles), (th, n)
      want = float(vals.mean()) if vals.size else 0.0
      assert got[th][n]['mean'] == pytest.approx(want, rel=1e-12, abs=1e-15), (th, n)
  assert any(got[th]['sbd']['mean'] > 0 for th in got) and got['0.30']['sbd']['count'] == 3
  # a flat-format archive whose images share one size gives the [N,Hf,Wf] archive's yaml
  x1, ids1 = _e2e_inputs()
  uniform = run('uniform', x=x1, names=np.array(NAMES), gt_instance_ids=ids1)
  assert run('uniform_flat', x=x1, names=np.array(NAMES), **setup_labels.flatten_images(list(ids1))) == uniform
  # with a foreground at the same offsets: the mask and the dilation act, per image
  rr, cc = np.mgrid[0:96, 0:80]
  fg1 = np.stack([((rr - 48) ** 2 / 40.0 ** 2 + (cc - 40 - 6 * n) ** 2 / 30.0 ** 2 <= 1).astype(np.uint8) for n in range(3)])
  with_fg = run('uniform_fg', '--remove_tiny', '60', x=x1, names=np.array(NAMES), gt_instance_ids=ids1, fg=fg1)
  assert run('uniform_flat_fg', '--remove_tiny', '60', x=x1, names=np.array(NAMES), fg_flat=fg1.reshape(-1),
             **setup_labels.flatten_images(list(ids1))) == with_fg and with_fg != uniform
  # refused by name on a mixed archive, before anything is restored
  mixed = str(tmp_path / 'mixed.npz')
  for flags in (['--render'], ['--render_gt_instances'], ['--fused_postprocess'], ['--cityscapes_output', str(tmp_path / 'cs'), '--fg_model_id', 'fg']):
    with pytest.raises(rn.RecAttendError, match='%s cannot be used with an --input of mixed full sizes' % flags[0]):
      full_model_eval.main(['--model_id', 'm0', '--results', res, '--input', mixed] + flags)
  bad = dict(flat, pixel_offset=flat['pixel_offset'].copy())
  bad['pixel_offset'][1] -= 8
  np.savez(str(tmp_path / 'bad.npz'), x=x, names=np.array(NAMES), **bad)
  with pytest.raises(rn.RecAttendError, match='image 0 is 96 x 80 at element 0, the next one starts at 7672'):
    full_model_eval.main(['--model_id', 'm0', '--results', res, '--input', str(tmp_path / 'bad.npz'), '--output', str(tmp_path / 'o')])


def test_fg_model_eval_on_mixed_sizes(cuda, tmp_path):
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
  size = np.array(SIZES, np.int32)

  def run(tag, *flags, **arrays):
    path, out = str(tmp_path / (tag + '.npz')), str(tmp_path / ('out_' + tag))
    np.savez(path, **arrays)
    fg_model_eval.main(['--model_id', 'fg', '--results', res, '--input', path, '--output', out, '--batch_size', '2', '--threshold_list',
                        '0.3,0.5', '--render_gt'] + list(flags))
    with open(os.path.join(out, 'metrics.yaml')) as f:
      return yaml.safe_load(f), out

  got, out = run('mixed', x=x, names=np.array(NAMES), fg_gt_full_flat=flat, pixel_offset=offset, orig_size=size)
  singles = [run('one%d' % i, x=x[i:i + 1], names=np.array(NAMES[i:i + 1]), fg_gt_full=gts[i][None])[0] for i in range(3)]
  for th in ('0.30', '0.50'):
    tot = {k: sum(s[th][k] for s in singles) for k in ('count_a', 'sum_ab', 'sum_b', 'pixels')}
    assert {k: got[th][k] for k in tot} == tot and tot['pixels'] == sum(h * w for h, w in SIZES)  # pixels summed per image
    inter, union = tot['sum_ab'], tot['count_a'] + tot['sum_b'] - tot['sum_ab']
    assert got[th]['fg_iou_all'] == pytest.approx(inter / union, rel=1e-12)
    b_inter = tot['pixels'] - tot['count_a'] - tot['sum_b'] + tot['sum_ab']
    b_union = (tot['pixels'] - tot['count_a']) + (tot['pixels'] - tot['sum_b']) - b_inter
    assert got[th]['bg_iou_all'] == pytest.approx(b_inter / b_union, rel=1e-12)
    for i, name in enumerate(NAMES):  # one PNG per image at its own size, the file the single-image run writes
      for folder in ('%02d' % int(float(th) * 100), 'gt'):
        img = png.read_gray8(os.path.join(out, folder, name))
        assert img.shape == SIZES[i]
        assert np.array_equal(img, png.read_gray8(os.path.join(str(tmp_path / ('out_one%d' % i)), folder, name)))
  # a flat-format archive whose images share one size gives the [N,H,W] archive's yaml
  g1 = feo.disc_labels(rng, 3, 96, 80)
  uniform, _ = run('uniform', x=x, names=np.array(NAMES), fg_gt_full=g1)
  as_flat, _ = run('uniform_flat', x=x, names=np.array(NAMES), fg_gt_full_flat=g1.reshape(-1), pixel_offset=np.arange(4, dtype=np.int64) * 7680,
                   orig_size=np.tile(np.array([[96, 80]], np.int32), (3, 1)))
  assert as_flat == uniform
  mixed = str(tmp_path / 'mixed.npz')
  with pytest.raises(rn.RecAttendError, match='--render_orientation cannot be used with an --input of mixed full sizes'):
    fg_model_eval.main(['--model_id', 'fg', '--results', res, '--input', mixed, '--render_orientation'])
  np.savez(str(tmp_path / 'px.npz'), x=x, fg_gt_full_flat=flat, pixel_offset=offset, orig_size=size, gt_instance_ids=np.zeros((3, 4, 4), np.int32))
  with pytest.raises(rn.RecAttendError, match=r'pixel-level class scores \(gt_instance_ids in --input\) cannot be computed on an --input of mixed'):
    fg_model_eval.main(['--model_id', 'fg', '--results', res, '--input', str(tmp_path / 'px.npz')])


def test_setup_labels_mixed_sizes(cuda, tmp_path):
  """A folder of label files of three sizes (+ their colour images): the archive holds the flat ids, the dense network-size
  labels and the flat full-size foreground, each image's equal to the oracle's on that image alone, and x equal to the resize
  of every image alone; the trainers assemble a batch from such an archive as from its images."""
  import full_model_train
  rng = np.random.RandomState(31)
  sizes = ((30, 50), (25, 35), (30, 50), (24, 40))
  labels, images = tmp_path / 'labels', tmp_path / 'images'
  labels.mkdir()
  images.mkdir()
  ids, colour = [], []
  for i, (h, w) in enumerate(sizes):
    ids.append(lo.ellipse_ids(np.random.RandomState(40 + i), 1, h, w, 4)[0])
    colour.append(rng.randint(0, 256, (h, w, 3)).astype(np.uint8))
    png.write_gray8(str(labels / ('%06d.png' % i)), ids[-1].astype(np.uint8))
    png.write_colour8(str(images / ('%06d.png' % i)), colour[-1])
  with pytest.raises(rn.RecAttendError, match='different sizes'):  # opt-in: the default refusal stands
    setup_labels.main(['--input', str(labels), '--dataset', 'kitti', '--height', '12', '--width', '20', '--timespan', '3', '--output',
                       str(tmp_path / 'no.npz')])
  out = str(tmp_path / 'fg_in.npz')
  setup_labels.main(['--input', str(labels), '--images', str(images), '--dataset', 'kitti', '--height', '12', '--width', '20', '--timespan',
                     '3', '--target', 'all', '--mixed_sizes', '--batch_size', '3', '--output', out])
  arch = dict(np.load(out))
  assert sorted(arch) == sorted(['y_gt_ins', 's_gt', 'c_gt', 'd_gt', 'd_cls', 'fg_gt_full_flat', 'inst_id', 'area', 'sem_cls', 'num_obj', 'names',
                                 'x', 'gt_instance_ids_flat', 'pixel_offset', 'orig_size'])
  assert arch['orig_size'].tolist() == [list(s) for s in sizes] and arch['pixel_offset'].tolist() == [0, 1500, 2376, 3876, 4836]
  assert arch['names'].tolist() == ['%06d.png' % i for i in range(4)]
  keys = {'y_gt_ins': 'y_gt', 's_gt': 's_gt', 'c_gt': 'c_gt', 'd_gt': 'd_gt', 'd_cls': 'd_cls', 'inst_id': 'inst_id', 'area': 'area',
          'sem_cls': 'sem_cls', 'num_obj': 'num_obj'}
  for i, (h, w) in enumerate(sizes):
    ref = lo.assemble(ids[i][None], 12, 20, 3, lo.PLAIN)
    assert ref['ori_margin'] >= 1e-6
    o = int(arch['pixel_offset'][i])
    assert np.array_equal(arch['gt_instance_ids_flat'][o:o + h * w].reshape(h, w), ids[i])
    assert np.array_equal(arch['fg_gt_full_flat'][o:o + h * w].reshape(h, w), ref['fg_gt_full'][0])
    for k, src in keys.items():
      assert np.array_equal(arch[k][i], ref[src][0]), (i, k)
    assert np.array_equal(arch['x'][i], ops.resize_cubic(colour[i][None], 12, 20, want=('x',))['x'][0].cpu().numpy()), i
  # the trainers: a batch in any order from the flat archive is the batch from its images
  idx = np.array([2, 0, 3])
  y_gt, s_gt = full_model_train.batch_labels({k: arch[k] for k in ('gt_instance_ids_flat', 'pixel_offset', 'orig_size', 'names')}, idx,
                                             12, 20, 3, 'kitti')
  assert np.array_equal(y_gt.cpu().numpy(), arch['y_gt_ins'][idx]) and np.array_equal(s_gt.cpu().numpy(), arch['s_gt'][idx])
