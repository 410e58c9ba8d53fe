"""The label stage on the MI355X: ra_ops.assemble_labels against the float64 oracle of the reference's stage
(tests/labels_oracle.py, the reference's list-of-masks formulation), the command line, and the two consumers — one training
step from assembled planes against the same step from ids, and fg_model_eval.py on --target fg_model output.

Every output is an integer, a 0 / 1 float or a class, so every comparison is array_equal.  The one place where rounding
could enter is the floor of the orientation value: the kernel and NumPy both evaluate it in double, in the same order,
and differ by a few ulp of asin / sqrt (1e-15 relative).  Before d_cls is compared the ORACLE's pre-floor value is asserted
to lie at least ORI_GUARD = 1e-6 from an integer on every foreground pixel of the input, nine orders above that; the seeds
below are chosen so that it does (checked without a device)."""
import functools
import os

import numpy as np
import pytest
import torch

import labels_oracle as lo
import ra_native as rn
import ra_ops as ops
from test_labels import cityscapes_id_image

pytestmark = pytest.mark.gpu
ORI_GUARD = 1e-6


def _tie_image():
  img = np.zeros((24, 40), np.int32)
  img[2:8, 2:10] = 11     # 6 x 8 at full size, 3 x 4 = 12 at network size
  img[12:20, 20:26] = 4   # 8 x 6 at full size, 4 x 3 = 12: the tie — id 11 (the larger catalogue index) goes first
  img[20:24, 30:40] = 7   # 4 x 10 -> 2 x 5 = 10
  return img


def _special_images(dataset):
  """[3,14,12] at ratio 2 -> 7 x 6: no accepted instance; one instance that no sampled position meets; the id list."""
  none = np.zeros((14, 12), np.int32)
  if dataset == lo.CITYSCAPES:
    none[:5], none[5:9, 2:8], none[10:, :6] = 7, 29001, 1000  # stuff, a caravan, an id that is not > 1000
  gone = np.zeros((14, 12), np.int32)
  gone[3, 5] = 26001 if dataset == lo.CITYSCAPES else 9
  return np.stack([none, gone, cityscapes_id_image()])


@functools.lru_cache(maxsize=None)
def case(name):
  """-> (gt_ids int32 [B,Hf,Wf], H, W, T, dataset)"""
  P, C = lo.PLAIN, lo.CITYSCAPES
  rs = np.random.RandomState
  table = {
      # integer ratio, truncation (6 instances, T = 4) and zero slots (3 instances, T = 8), both rules
      'int_trunc_plain': lambda: (lo.ellipse_ids(rs(1), 2, 24, 40, 6), 12, 20, 4, P),
      'int_trunc_cs': lambda: (lo.ellipse_ids(rs(1), 2, 24, 40, 7, C), 12, 20, 4, C),  # the seventh is a caravan
      'int_zero_plain': lambda: (lo.ellipse_ids(rs(1), 2, 24, 40, 3), 12, 20, 8, P),
      'int_zero_cs': lambda: (lo.ellipse_ids(rs(1), 2, 24, 40, 4, C), 12, 20, 8, C),
      # non-integer ratios: 2.5, and 25 / 12 x 35 / 20 (the min(.., Hf - 1) clamp is in force)
      'ratio_2p5': lambda: (lo.ellipse_ids(rs(5), 2, 30, 50, 5), 12, 20, 6, P),
      'ratio_odd': lambda: (lo.ellipse_ids(rs(6), 2, 25, 35, 5, C), 12, 20, 6, C),
      # ratio 1: W % 4 != 0 with H * W % 4 == 0 (vector stores whose 4 pixels straddle rows), and H * W % 4 != 0 (element stores)
      'unaligned_w': lambda: (lo.ellipse_ids(rs(7), 2, 12, 18, 4), 12, 18, 5, P),
      'unaligned_hw': lambda: (lo.ellipse_ids(rs(8), 2, 13, 18, 4, C), 13, 18, 5, C),
      'unaligned_hw_plain': lambda: (lo.ellipse_ids(rs(9), 1, 11, 9, 3), 11, 9, 3, P),
      'special_plain': lambda: (_special_images(P), 7, 6, 8, P),
      'special_cs': lambda: (_special_images(C), 7, 6, 8, C),
      'tie': lambda: (np.stack([_tie_image(), _tie_image()[::-1].copy()]), 12, 20, 4, P),
      # several workgroups per image leave partial moments, a few dozen instances, T at its cap
      'multi_wg': lambda: (lo.ellipse_ids(rs(10), 3, 64, 96, 40, C, 0.03, 0.12), 64, 96, 32, C),
      'multi_wg_plain': lambda: (lo.ellipse_ids(rs(11), 3, 64, 96, 40, P, 0.03, 0.12), 64, 96, 20, P),
  }
  gt, H, W, T, dataset = table[name]()
  return np.ascontiguousarray(gt, np.int32), H, W, T, dataset


CASES = ('int_trunc_plain', 'int_trunc_cs', 'int_zero_plain', 'int_zero_cs', 'ratio_2p5', 'ratio_odd', 'unaligned_w', 'unaligned_hw',
         'unaligned_hw_plain', 'special_plain', 'special_cs', 'tie', 'multi_wg', 'multi_wg_plain')


@functools.lru_cache(maxsize=None)
def reference(name):
  gt, H, W, T, dataset = case(name)
  return lo.assemble(gt, H, W, T, dataset)


def _dev(gt):
  return torch.from_numpy(np.ascontiguousarray(gt, np.int32)).cuda()


def _assert_equal(got, ref, what, images=None):
  for k in lo.KEYS:
    g, r = got[k].cpu().numpy(), ref[k]
    if images is not None:
      g, r = g[images], r[images]
    assert g.dtype == r.dtype and g.shape == r.shape, (what, k, g.dtype, r.dtype, g.shape, r.shape)
    bad = int((g != r).sum())
    print('%s %-10s %s %s: %d of %d differ' % (what, k, g.dtype, g.shape, bad, g.size))
    assert bad == 0, (what, k, bad)


@pytest.mark.parametrize('name', CASES)
def test_assemble_labels_matches_oracle(cuda, name):
  gt, H, W, T, dataset = case(name)
  ref = reference(name)
  print('%s: orientation margin of the oracle %.3g' % (name, ref['ori_margin']))
  assert ref['ori_margin'] >= ORI_GUARD  # a condition on the input
  got = ops.assemble_labels(_dev(gt), H, W, T, dataset, want=ops.LABEL_OUTPUTS)
  _assert_equal(got, ref, name)
  if name.startswith('int_trunc'):  # truncation: every slot is taken and the orientation covers the instances left out
    assert (ref['num_obj'] == 6).all() and T == 4 and (ref['s_gt'] == 1).all()
    assert (ref['d_cls'][ref['y_gt'].max(axis=1) == 0] > 0).any()
  if name.startswith('int_zero'):
    assert (ref['num_obj'] == 3).all() and T == 8 and not ref['y_gt'][:, 3:].any()
  if name == 'tie':
    assert ref['inst_id'][0].tolist() == [11, 4, 7, -1] and ref['area'][0].tolist() == [12, 12, 10, 0]
  if name.startswith('special'):
    assert ref['num_obj'][:2].tolist() == [0, 1] and ref['s_gt'][1].tolist() == [1] + [0] * 7 and not ref['y_gt'][1].any()
  if name.startswith('multi_wg'):
    assert ref['num_obj'].min() >= 24 and H * W > 4 * 256


def test_numpy_input_and_partial_want(cuda):
  gt, H, W, T, dataset = case('ratio_odd')
  ref = reference('ratio_odd')
  got = ops.assemble_labels(gt.astype(np.uint16), H, W, T, 'cityscapes', want=('d_gt', 'area'))
  assert sorted(got) == ['area', 'd_gt'] and got['d_gt'].is_cuda
  assert np.array_equal(got['d_gt'].cpu().numpy(), ref['d_gt']) and np.array_equal(got['area'].cpu().numpy(), ref['area'])
  only_fg = ops.assemble_labels(_dev(gt), H, W, T, dataset, want=('fg_gt_full',))
  assert np.array_equal(only_fg['fg_gt_full'].cpu().numpy(), ref['fg_gt_full'])
  with pytest.raises(rn.RecAttendError, match='want'):
    ops.assemble_labels(_dev(gt), H, W, T, dataset, want=('y_gt', 'boxes'))
  with pytest.raises(rn.RecAttendError, match='T=33'):
    ops.assemble_labels(_dev(gt), H, W, 33, dataset)
  with pytest.raises(rn.RecAttendError, match='int32'):
    ops.assemble_labels(_dev(gt).to(torch.int64), H, W, T, dataset)


def test_run_to_run_identical(cuda):
  gt, H, W, T, dataset = case('multi_wg')
  d = _dev(gt)
  a = ops.assemble_labels(d, H, W, T, dataset, want=ops.LABEL_OUTPUTS)
  b = ops.assemble_labels(d, H, W, T, dataset, want=ops.LABEL_OUTPUTS)
  for k in ops.LABEL_OUTPUTS:
    assert a[k].cpu().numpy().tobytes() == b[k].cpu().numpy().tobytes(), k


def test_catalogue_overflow_names_the_image_and_spares_the_others(cuda):
  gt0 = case('int_trunc_plain')[0][0]
  many = np.zeros_like(gt0)
  many.reshape(-1)[:257] = np.arange(1, 258)  # 257 ids and the background
  gt = np.stack([gt0, many])
  with pytest.raises(rn.RecAttendError, match=r'image 1 has more than 256 distinct instance ids'):
    ops.assemble_labels(_dev(gt), 12, 20, 4, 'cvppp', want=ops.LABEL_OUTPUTS)
  with pytest.raises(rn.RecAttendError, match=r'image b\.png has more than 256'):
    ops.assemble_labels(_dev(gt), 12, 20, 4, 'cvppp', names=['a.png', 'b.png'])
  d = _dev(gt)
  ids, pixels, count, status = ops.gt_instance_catalog(d, check_status=False)
  got = ops.assemble_labels_raw(d, (ids, pixels, count), 12, 20, 4, 'cvppp')
  assert status.cpu().tolist() == [0, rn.RA_GT_STATUS_COUNT]
  _assert_equal(got, reference('int_trunc_plain'), 'image 0 beside an overflowing image', images=slice(0, 1))
  bad = gt.copy()
  bad[1, 0, 0] = 70000  # outside the 16-bit range
  with pytest.raises(rn.RecAttendError, match=r'image 1 has an instance id outside'):
    ops.assemble_labels(_dev(bad), 12, 20, 4, 'cvppp')


ARCH = ['--ctrl_cnn_filter_size', '3,3,3,3,3', '--ctrl_cnn_depth', '8,8,16,16,32', '--ctrl_cnn_pool', '2,2,2,2,2', '--attn_cnn_filter_size',
        '3,3,3', '--attn_cnn_depth', '8,8,16', '--attn_cnn_pool', '2,2,2', '--attn_dcnn_filter_size', '3,3,3,3', '--attn_dcnn_depth',
        '16,8,8,1', '--attn_dcnn_pool', '2,2,2,1', '--stop_canvas_grad', '--fixed_gamma', '--ctrl_add_inp', '--ctrl_add_canvas',
        '--attn_add_inp', '--attn_add_canvas', '--base_learn_rate', '0.001']


def test_training_step_from_ids_equals_step_from_assembled_planes(cuda, tmp_path):
  """setup_labels.py --target full_model, one full_model_train.py step from its output, and the same step straight from the
  ids: the same loss to the bit.  (On the parent commit the second run ends in KeyError 'y_gt'.)"""
  import full_model_train
  import setup_labels
  rng = np.random.RandomState(21)
  ids = lo.ellipse_ids(rng, 2, 64, 64, 3, lo.PLAIN, 0.1, 0.3)
  x = rng.rand(2, 64, 64, 3).astype(np.float32)
  from_ids, planes, res = str(tmp_path / 'ids.npz'), str(tmp_path / 'planes.npz'), str(tmp_path / 'results')
  np.savez(from_ids, gt_instance_ids=ids, x=x, names=np.array(['a.png', 'b.png']))
  setup_labels.main(['--input', from_ids, '--dataset', 'cvppp', '--height', '64', '--width', '64', '--timespan', '2', '--target',
                     'full_model', '--output', planes])
  ref = lo.assemble(ids, 64, 64, 2, lo.PLAIN)
  made = dict(np.load(planes))
  assert sorted(made) == ['s_gt', 'x', 'y_gt'] and np.array_equal(made['y_gt'], ref['y_gt']) and np.array_equal(made['s_gt'], ref['s_gt'])
  assert np.array_equal(made['x'], x) and ref['y_gt'][:, 1].any()
  common = ['--results', res, '--batch_size', '2', '--inp_height', '64', '--inp_width', '64', '--timespan', '2', '--padding', '0',
            '--dataset', 'cvppp', '--seed', '7', '--save_rank_weights'] + ARCH
  full_model_train.main(['--init_only', '--model_id', 'init'] + common)
  losses = []
  for model_id, src in (('planes', planes), ('ids', from_ids)):
    full_model_train.main(['--restore', os.path.join(res, 'init'), '--num_steps', '1', '--model_id', model_id, '--input', src] + common)
    losses.append(np.load(os.path.join(res, model_id, 'weights_rank0.npz'))['loss_history'])
  print('loss from planes %r, from ids %r' % (losses[0].tolist(), losses[1].tolist()))
  assert losses[0].shape == (1,) and np.isfinite(losses[0]).all() and losses[0].tobytes() == losses[1].tobytes()


def test_fg_model_eval_on_assembled_ground_truth(cuda, tmp_path, capsys):
  """setup_labels.py --target fg_model feeds fg_model_eval.py, which reports the orientation statistics; and
  fg_model.Model.statistics on the assembled y_gt / d_gt equals tests/fg_eval_oracle.py on the ORACLE's arrays within the
  bounds tests/test_fg_eval_gpu.py holds that method to."""
  import yaml
  import fg_eval_oracle as feo
  import fg_model
  import fg_model_eval
  import fg_oracle as fo
  import setup_labels
  import test_fg_eval_gpu as tfe
  opt = dict(fo.reduced_opt(1, True), segm_loss_fn='bce')
  P = fo.random_weights(opt, 71)
  res = str(tmp_path / 'results')
  os.makedirs(os.path.join(res, 'fg'))
  with open(os.path.join(res, 'fg', 'model_opt.yaml'), 'w') as f:
    yaml.safe_dump(opt, f)
  np.savez(os.path.join(res, 'fg', 'weights.npz'), step=np.float32(1), **P)
  rng = np.random.RandomState(72)
  N, h, w, Hf, Wf = 2, 32, 48, 64, 96
  ids = lo.ellipse_ids(rng, N, Hf, Wf, 5)
  x = rng.rand(N, h, w, 3).astype(np.float32)
  src, made = str(tmp_path / 'ids.npz'), str(tmp_path / 'fg_in.npz')
  np.savez(src, gt_instance_ids=ids, x=x, names=np.array(['a.png', 'b.png']))
  setup_labels.main(['--input', src, '--dataset', 'kitti', '--height', str(h), '--width', str(w), '--timespan', '4', '--target',
                     'fg_model', '--output', made])
  ref = lo.assemble(ids, h, w, 4, lo.PLAIN)
  assert ref['ori_margin'] >= ORI_GUARD
  arch = dict(np.load(made))
  assert sorted(arch) == ['d_gt', 'fg_gt_full', 'names', 'x', 'y_gt']
  assert np.array_equal(arch['y_gt'], ref['c_gt']) and np.array_equal(arch['d_gt'], ref['d_gt'])
  assert np.array_equal(arch['fg_gt_full'], ref['fg_gt_full']) and arch['fg_gt_full'].dtype == np.uint8
  capsys.readouterr()
  out = str(tmp_path / 'out')
  met = fg_model_eval.main(['--model_id', 'fg', '--results', res, '--input', made, '--output', out, '--batch_size', '2'])
  text = capsys.readouterr().out
  assert 'orientation_ce' in text and 'orientation_acc' in text
  stats = met['statistics']
  assert np.isfinite(stats['orientation_ce']) and 0.0 <= stats['orientation_acc'] <= 1.0
  # the statistics of the model on the assembled arrays against the float64 oracle on the oracle's arrays
  fwd = fo.forward(opt, P, x)
  s, bound = tfe._propagated(fwd, ref['c_gt'], ref['d_gt'], 1, 8, float(N * h * w), 'bce')
  want = feo.statistics_of(s, float(N * h * w), 'bce', True)
  m = fg_model.get_model(opt).load_weights(P)
  got = m.statistics(tfe._dev(x), tfe._dev(arch['y_gt']), tfe._dev(arch['d_gt']))
  assert set(got) == set(want)
  for k in sorted(want):
    err = abs(got[k] - want[k])
    print('%-16s got %.8g ref %.8g |err| %.3g (propagated bound %.3g)' % (k, got[k], want[k], err, bound[k]))
    assert err <= bound[k] + tfe.FLOOR, (k, got[k], want[k], bound[k])
    assert stats[k] == pytest.approx(got[k], rel=1e-12, abs=1e-12)  # one batch: the CLI's mean is that batch's value
