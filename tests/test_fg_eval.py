"""Evaluating the pre-stage without a GPU: the float64 oracle of fg_model.py:196-246 on hand-worked cases, the whole-dataset
IoU analyzers on integer counters, the flag surface of fg_model_eval.py, the exported symbols and the argument checks."""
import math

import numpy as np
import pytest
import torch

import analysis
import cmd_args_parser as cap
import fg_eval_oracle as feo
import fg_model_eval
import ra_native as rn
import ra_ops as ops

L2, L3, L9 = math.log(2.0), math.log(3.0), math.log(9.0)
E = 1e-5


def _close(got, want):
  assert set(got) == set(want)
  for k in want:
    assert got[k] == pytest.approx(want[k], rel=1e-12, abs=1e-12), k


# ---- the oracle, one class: sigmoid(0) = .5, sigmoid(ln 3) = .75, sigmoid(-ln 3) = .25, sigmoid(ln 9) = .9
def test_oracle_one_class_by_hand():
  lg = np.array([[0.0, L3], [-L3, L9]]).reshape(1, 2, 2, 1)
  g = np.array([[1.0, 1.0], [0.0, 0.0]]).reshape(1, 2, 2)
  s = feo.sums(lg, g, None, 1, 0)
  bce = -math.log(.5 + E) - math.log(.75 + E) - math.log(1 - .25 + E) - math.log(1 - .9 + E)
  _close(s, {'inter_soft': .5 + .75, 'sum_soft': .5 + .75 + .25 + .9, 'sum_gt': 2.0,
             'inter_hard': 1.0,  # y = .5 is not > .5: pixel 0 is not hard; pixels 1 and 3 are, pixel 1 carries g
             'sum_hard': 2.0, 'seg_ce': bce, 'ori_ce': 0.0, 'ori_correct': 0.0, 'mask': 0.0})
  iou_soft, iou_hard = 1.25 / (2.4 + 2 - 1.25 + E), 1.0 / (2 + 2 - 1 + E)
  _close(feo.statistics(lg, g, None, 1, 0, 'iou'), {'iou_soft': iou_soft, 'iou_hard': iou_hard, 'foreground_loss': -iou_soft,
                                                    'loss': -iou_soft})
  _close(feo.statistics(lg, g, None, 1, 0, 'bce'), {'iou_soft': iou_soft, 'iou_hard': iou_hard, 'foreground_loss': bce / 4,
                                                    'loss': bce / 4})


def test_oracle_empty_mask_gives_nan():
  lg = np.zeros((1, 2, 2, 9))
  lg[..., 0] = [[0.0, L3], [-L3, L9]]
  d_gt = np.zeros((1, 2, 2, 8))
  d_gt[..., 3] = 1
  st = feo.statistics(lg, np.zeros((1, 2, 2)), d_gt, 1, 8, 'bce')
  assert math.isnan(st['orientation_acc']) and math.isnan(st['orientation_ce']) and math.isnan(st['loss'])
  assert st['iou_soft'] == 0.0 and st['iou_hard'] == 0.0
  bce = -math.log(1 - .5 + E) - math.log(1 - .75 + E) - math.log(1 - .25 + E) - math.log(1 - .9 + E)
  assert st['foreground_loss'] == pytest.approx(bce / 4, rel=1e-12)


# ---- three classes with orientation
#   pixel  class logits     softmax          g      hard           orientation logits      d softmax      d_gt
#   0      0, ln2, ln2      .2 .4 .4         c1     c1 AND c2      0,ln2,ln2,0..           .1 .2 .2 .1..  idx 1   (tie: first wins -> 1, correct)
#   1      ln2, 0, 0        .5 .25 .25       c0     c0             0..                     1/8 each       idx 0   (correct, but mask 0)
#   2      0, 0, ln2        .25 .25 .5       c2     c2             ln3,0..                 .3 .1 ..       idx 4   (wrong)
#   3      0, ln3, 0        .2 .6 .2         c2     c1             0..                     1/8 each       .5 .5 0.. (tie: first wins -> 0, correct)
def test_oracle_three_classes_with_orientation_by_hand():
  cls = np.array([[0, L2, L2], [L2, 0, 0], [0, 0, L2], [0, L3, 0]], np.float64)
  ori = np.zeros((4, 8))
  ori[0, 1] = ori[0, 2] = L2
  ori[2, 0] = L3
  lg = np.concatenate([cls, ori], axis=1).reshape(1, 2, 2, 11)
  g = np.array([[0, 1, 0], [1, 0, 0], [0, 0, 1], [0, 0, 1]], np.float64).reshape(1, 2, 2, 3)
  d_gt = np.zeros((4, 8))
  d_gt[0, 1] = 1
  d_gt[1, 0] = 1
  d_gt[2, 4] = 1
  d_gt[3, 0] = d_gt[3, 1] = .5
  d_gt = d_gt.reshape(1, 2, 2, 8)
  ce = -math.log(.4 + E) - math.log(.5 + E) - math.log(.5 + E) - math.log(.2 + E)  # all channels: pixel 1's background too
  ori_ce = -math.log(.2 + E) - math.log(.1 + E) - 2 * .5 * math.log(.125 + E)      # pixels 0, 2, 3; pixel 1 is masked
  want = {'inter_soft': .4 + 0 + .5 + .2, 'sum_soft': .8 + .5 + .75 + .8, 'sum_gt': 3.0,
          'inter_hard': 1.0 + 0 + 1.0 + 0,  # pixel 0: c1 hard and labelled; pixel 3: c1 hard, c2 labelled
          'sum_hard': 2.0 + 0 + 1.0 + 1.0,  # pixel 0 counts in BOTH channels
          'seg_ce': ce, 'ori_ce': ori_ce, 'ori_correct': 2.0, 'mask': 3.0}
  _close(feo.sums(lg, g, d_gt, 3, 8), want)
  iou_soft, iou_hard = 1.1 / (2.85 + 3 - 1.1 + E), 2.0 / (4 + 3 - 2 + E)
  _close(feo.statistics(lg, g, d_gt, 3, 8, 'bce'),
         {'iou_soft': iou_soft, 'iou_hard': iou_hard, 'foreground_loss': ce / 4, 'orientation_ce': ori_ce / 3,
          'orientation_acc': 2.0 / 3, 'loss': ce / 4 + ori_ce / 3})
  assert feo.statistics(lg, g, d_gt, 3, 8, 'iou')['loss'] == pytest.approx(-iou_soft + ori_ce / 3, rel=1e-12)


def test_oracle_upsample_is_pp_upsample():
  import ra_oracle as ora
  rng = np.random.RandomState(8)
  for (Hs, Ws, H, W) in ((6, 9, 13, 17), (8, 12, 5, 7), (4, 4, 3, 3)):
    src = rng.rand(2, Hs, Ws)
    assert np.array_equal(feo.upsample(src, H, W), ora.pp_upsample(src, H, W))
  one = feo.upsample(rng.rand(1, 1, 1), 1, 4)  # a single row: every neighbour in y is the row itself
  assert one.shape == (1, 1, 4) and np.allclose(one, one[0, 0, 0])


# ---- the analyzers on integer counters
def _counts(a, b):
  return {'count_a': a.sum(axis=(1, 2))[:, None], 'sum_ab': (a * b).sum(axis=(1, 2))[:, None], 'sum_b': b.sum(axis=(1, 2)),
          'pixels': a.shape[1] * a.shape[2]}


def test_analyzers_accumulate_over_stage_calls(capsys):
  rng = np.random.RandomState(3)
  a = (rng.rand(5, 6, 9) > 0.4).astype(np.int64)
  b = rng.randint(0, 3, (5, 6, 9)).astype(np.int64)  # values of 2: overlapping instances
  assert (b == 2).any()
  fg, bg = analysis.ForegroundIOUAnalyzer(), analysis.BackgroundIOUAnalyzer()
  for sl in (slice(0, 2), slice(2, 5)):
    for an in (fg, bg):
      an.stage({'fg_counts': _counts(a[sl], b[sl])})
  got_fg, got_bg = fg.finalize(), bg.finalize()
  out = capsys.readouterr().out.splitlines()
  assert out == ['{:17s}{:7.4f}'.format('FG IOU ALL', got_fg), '{:17s}{:7.4f}'.format('BG IOU ALL', got_bg)]
  assert isinstance(got_fg, float) and got_fg == pytest.approx(feo.fg_iou_all(list(a), list(b)), rel=1e-15)
  assert got_bg == pytest.approx(feo.bg_iou_all(list(a), list(b)), rel=1e-15)
  # binary labels: the closed forms of the background
  b1 = np.minimum(b, 1)
  bg = analysis.BackgroundIOUAnalyzer()
  bg.stage({'fg_counts': _counts(a, b1)})
  hw, ca, sb, sab = a.size, int(a.sum()), int(b1.sum()), int((a * b1).sum())
  assert (bg.inter, bg.union) == (hw - ca - sb + sab, hw - sab)


def test_analyzers_pick_their_threshold_and_are_not_registered():
  c = {'count_a': np.array([[10, 4]]), 'sum_ab': np.array([[6, 3]]), 'sum_b': np.array([8]), 'pixels': 20}
  f0, f1 = analysis.ForegroundIOUAnalyzer(index=0), analysis.ForegroundIOUAnalyzer(index=1)
  f0.stage({'fg_counts': c}), f1.stage({'fg_counts': c})
  assert (f0.inter, f0.union, f1.inter, f1.union) == (6, 12, 3, 9)
  assert 'fg_iou_all' not in analysis.ANALYZERS and 'bg_iou_all' not in analysis.ANALYZERS
  assert math.isnan(analysis.ForegroundIOUAnalyzer().finalize())
  with pytest.raises(rn.RecAttendError):
    analysis.ForegroundIOUAnalyzer().stage({'y_out': torch.zeros(1, 2, 2), 'y_gt': torch.zeros(1, 2, 2)})  # CPU tensors


# ---- the flag surface
def test_flag_table():
  names = [n for n, _, _ in cap.FG_EVAL_FLAGS]
  assert set(names) == {'threshold_list', 'render_ori', 'render_soft', 'render_gt', 'model_id', 'batch_size', 'results', 'output',
                        'split', 'prefetch', 'queue_size', 'num_worker'} and len(names) == len(set(names))
  p = fg_model_eval.build_parser()
  args = p.parse_args(['--model_id', 'fg'])
  assert (args.batch_size, args.results, args.output, args.threshold_list) == (32, './results', None, None)
  opt = fg_model_eval.make_opt(args)
  assert opt['threshold_list'] == [0.3] and opt['split'] == ['valid'] and not opt['render_soft'] and not opt['render_gt']
  opt = fg_model_eval.make_opt(p.parse_args(['--threshold_list', '0.5,0.1', '--render_soft', '--render_gt']))
  assert opt['threshold_list'] == [0.5, 0.1] and opt['render_soft'] and opt['render_gt']
  with pytest.raises(rn.RecAttendError, match='orientation'):
    fg_model_eval.make_opt(p.parse_args(['--render_ori']))
  with pytest.raises(Exception, match='model ID'):
    fg_model_eval.main(['--input', 'nothing.npz'])


def test_symbols_are_exported():
  lib = rn.lib()
  for name in ('ra_fg_stats_workspace_bytes', 'ra_fg_stats_f32', 'ra_fg_sweep_counts_f32'):
    assert name in rn.SIGNATURES and hasattr(lib, name)
  assert rn.RA_FG_STAT_COUNT == len(ops.FG_STAT_NAMES) == len(feo.SUM_NAMES) and ops.FG_STAT_NAMES == feo.SUM_NAMES
  assert [getattr(rn, 'RA_FG_STAT_' + n.upper()) for n in ops.FG_STAT_NAMES] == list(range(rn.RA_FG_STAT_COUNT))
  assert rn.RA_FG_SWEEP_MAX_K == 16 and rn.RA_FG_SWEEP_SLOTS == 2 * 16 + 1
  assert lib.ra_fg_stats_workspace_bytes(0) == 0
  assert lib.ra_fg_stats_workspace_bytes(1) == 9 * 8 and lib.ra_fg_stats_workspace_bytes(257) == 2 * 9 * 8


def test_argument_validation_without_a_device():
  z = torch.zeros
  u8 = lambda *s: torch.zeros(*s, dtype=torch.uint8)
  with pytest.raises(rn.RecAttendError, match='17 thresholds'):
    ops.fg_sweep_counts(z(1, 2, 2), u8(1, 2, 2), [0.1] * 17)
  with pytest.raises(rn.RecAttendError, match='0 thresholds'):
    ops.fg_sweep_counts(z(1, 2, 2), u8(1, 2, 2), [])
  with pytest.raises(rn.RecAttendError, match='nsc 17'):
    ops.fg_statistics(z(4, 17), z(4, 17), None, 17, 0)
  with pytest.raises(rn.RecAttendError, match='no 3'):
    ops.fg_statistics(z(4, 4), z(4, 1), z(4, 3), 1, 3)
  with pytest.raises(rn.RecAttendError, match='CPU tensor'):
    ops.fg_statistics(z(4, 1), z(4, 1), None, 1, 0)
  with pytest.raises(rn.RecAttendError, match='CPU tensor'):
    ops.fg_sweep_counts(z(1, 2, 2), u8(1, 2, 2), [0.3])
  with pytest.raises(rn.RecAttendError, match='d_gt'):
    ops.fg_statistics(z(4, 1), z(4, 1), z(4, 8), 1, 0)
  # the C entry points refuse before any launch, too
  lib = rn.lib()
  buf = np.zeros(64, np.float64)
  p = buf.ctypes.data
  assert lib.ra_fg_stats_f32(p, p, None, 4, 17, 0, p, 512, p, None) == rn.RA_E_SHAPE
  assert lib.ra_fg_stats_f32(p, p, p, 4, 1, 3, p, 512, p, None) == rn.RA_E_SHAPE
  assert lib.ra_fg_stats_f32(p, p, None, 4, 1, 8, p, 512, p, None) == rn.RA_E_INVALID  # orientation without d_gt
  assert lib.ra_fg_stats_f32(p, p, None, 4, 1, 0, p, 8, p, None) == rn.RA_E_WORKSPACE
  assert lib.ra_fg_sweep_counts_f32(p, p, 1, 2, 2, 2, 2, p, 17, p, None) == rn.RA_E_SHAPE
  assert lib.ra_fg_sweep_counts_f32(p, p, 1, 2, 2, 2, 2, p, 0, p, None) == rn.RA_E_SHAPE
  assert lib.ra_fg_sweep_counts_f32(p, None, 1, 2, 2, 2, 2, p, 1, p, None) == rn.RA_E_INVALID


def test_model_statistics_refuses_before_any_launch():
  import fg_model
  import fg_oracle as fo
  m = fg_model.get_model(fo.reduced_opt(nsc=1, orientation=False))
  x = torch.zeros(1, 8, 8, 3)
  with pytest.raises(rn.RecAttendError, match='device tensor'):
    m.statistics(x, torch.zeros(1, 8, 8))
  with pytest.raises(rn.RecAttendError, match='eval only'):
    m.run(['loss'], {'x': x, 'phase_train': False})
