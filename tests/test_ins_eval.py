"""The evaluator from instance-id images, without a device: the float64 oracle's two routes agree (counts -> metrics against
ra_oracle.eval_metrics on the materialised masks, 1e-12), the conditions under which the band of tests/ins_eval_oracle.py says
anything hold for every case the GPU test runs, a NumPy mutant of each rule of the pass is rejected by some case, and the
refusals of ra_ops, of the C entry point and of the command line that need no device."""
import functools

import numpy as np
import pytest
import torch

import ins_eval_oracle as ieo
import ra_native as rn
import ra_ops as ops
import ra_oracle as ora

ROUTE_TOL = 1e-12


@functools.lru_cache(maxsize=None)
def _case(name):
  return ieo.make_case(name)


@functools.lru_cache(maxsize=None)
def _values(name, morph, mutant=None):
  Hf, Wf = ieo.CASES[name][4:6]
  return ieo.values(_case(name)['yc'], Hf, Wf, morph, mutant)


def tie_case():
  """b1_t3_16x16_16x16 with instance 2 a copy of instance 0: exact ties at every pixel instance 0 would win."""
  c = dict(_case('b1_t3_16x16_16x16'))
  yc = c['yc'].copy()
  yc[:, 2] = yc[:, 0]
  c['yc'] = yc
  return c


@pytest.mark.parametrize('name', ['b2_t5_24x40_61x103', 'b1_t3_16x16_16x16', 'b3_t2_4x4_2x3', 'b1_t1_1x1_1x4'])
@pytest.mark.parametrize('morph', [False, True])
@pytest.mark.parametrize('with_fg', [False, True])
def test_counts_route_equals_masks_route(name, morph, with_fg):
  c, v = _case(name), _values(name, morph)
  fg = c['fg'] if with_fg else None
  y_gt = ieo.gt_planes(c['gt_ids'], c['inst_id']).astype(np.float64)  # float32 planes would have eval_metrics sum in float32
  s_gt = c['s_gt'].astype(np.float64)  # likewise: 1 / num_obj
  thresholds = ieo.THRESHOLDS[10]
  inter, area_b = ieo.counts(v, c['gt_ids'], c['inst_id'], thresholds, fg)
  assert (area_b == y_gt.sum(axis=(2, 3))).all()
  conf = (np.arange(c['inst_id'].size).reshape(c['inst_id'].shape) % 3 > 0).astype(np.float64)
  for k, th in enumerate(thresholds):
    y = ieo.masks(v, th, fg)
    assert (inter[:, k].sum(axis=2) == y.sum(axis=(2, 3))).all()  # a prediction's area is its row sum
    for tiny in (0, int(np.median(inter[:, k].sum(axis=2)))):
      cnt, cf = ieo.apply_remove_tiny(inter[:, k], conf, tiny)
      y2, cf2 = ora.pp_remove_tiny(y, conf, tiny)
      assert (cf == cf2).all()
      got, ref = ieo.metrics_from_counts(cnt, area_b, s_gt), ora.eval_metrics(y2, y_gt, s_gt)
      assert set(got) == set(ref)
      for key in ref:
        assert got[key].shape == ref[key].shape, key
        assert np.abs(got[key] - ref[key]).max(initial=0) <= ROUTE_TOL, (name, th, tiny, key)


@pytest.mark.parametrize('name', sorted(ieo.CASES))
def test_band_conditions_hold_for_every_gpu_case(name):
  c = _case(name)
  for morph in (False, True):
    v = _values(name, morph)
    for K in (1, 10, 16):
      for fg in (None, c['fg']):
        lo, hi, share, ties = ieo.conditions(v, c['gt_ids'], c['inst_id'], ieo.THRESHOLDS[K], fg)
        print('%s morph %d K %2d fg %d: undecided share %.5f, band %d counts, exact ties %d' % (
            name, morph, K, fg is not None, share, int((hi - lo).sum()), ties))
        assert share <= ieo.BAND_SHARE and ties == 0
        assert (lo <= hi).all()
        full = ieo.counts(v, c['gt_ids'], c['inst_id'], ieo.THRESHOLDS[K], fg)[0]
        assert (lo <= full).all() and (full <= hi).all()
        if (name in ieo.EMPTY_BAND and K in (1, 10)) or name in ieo.EDGE_CASES:
          assert (lo == hi).all()  # these hold the device to the oracle's counts exactly


def test_tie_case_is_decided_but_for_the_copy():
  """Without the copied instance the tie case has an empty band: on the device, where equal inputs give equal values, only the
  order of the instances decides the rest."""
  c = tie_case()
  v = ieo.values(c['yc'][:, :2], 16, 16, False)
  for K in (1, 10, 16):
    lo, hi, share, ties = ieo.conditions(v, c['gt_ids'], c['inst_id'][:, :2], ieo.THRESHOLDS[K], None)
    assert (lo == hi).all() and ties == 0
  v3 = ieo.values(c['yc'], 16, 16, False)
  assert (v3[:, 2] == v3[:, 0]).all() and ieo.counts(v3, c['gt_ids'], c['inst_id'], [0.0])[0][:, :, 2].sum() == 0


def _rejected(name, morph, K, mutant_values=None, mutant_masks=None, case=None):
  c = case or _case(name)
  Hf, Wf = ieo.CASES[name][4:6]
  v = ieo.values(c['yc'], Hf, Wf, morph)
  if case is None:
    lo, hi, _, _ = ieo.conditions(v, c['gt_ids'], c['inst_id'], ieo.THRESHOLDS[K], None)
  else:  # exact ties: the oracle's own counts are the bar
    lo = hi = ieo.counts(v, c['gt_ids'], c['inst_id'], ieo.THRESHOLDS[K])[0]
  vm = ieo.values(c['yc'], Hf, Wf, morph, mutant_values) if mutant_values else v
  got = ieo.counts(vm, c['gt_ids'], c['inst_id'], ieo.THRESHOLDS[K], None, mutant_masks)[0]
  return bool(((got < lo) | (got > hi)).any())


def test_every_rule_has_a_case_that_rejects_its_mutant():
  assert _rejected('b1_t3_16x16_16x16', False, 10, mutant_masks='last_max', case=tie_case())  # last maximum in place of first
  assert not _rejected('b1_t3_16x16_16x16', False, 10, case=tie_case())
  assert _rejected('b2_t4_8x12_37x50', False, 10, mutant_masks='ge')             # >= in place of >: the zeros pass 0.0
  assert _rejected('b2_t5_24x40_61x103', True, 10, mutant_values='morph_first')  # the dilation in front of the filter
  assert _rejected('b2_t5_24x40_61x103', True, 10, mutant_values='radius1')      # a 3 x 3 window in place of 5 x 5
  assert not _rejected('b2_t5_24x40_61x103', True, 10)


def test_a_reflected_border_cannot_be_told_from_an_ignored_one():
  """The fourth mutant one would want — the image border reflected into the dilation's window instead of ignored — is no
  mutant: BORDER_REFLECT_101 maps the offsets -1, -2 to +1, +2, which the 5 x 5 window of a border pixel holds anyway (from 3
  rows and columns on), and a maximum does not count how often it sees a value.  Held here, so that nobody looks for a case
  that tells the two apart; the rule that CAN go wrong on the device — a value of the tile's halo that lies outside the image
  entering the maximum — is what the one-pixel-over-the-tile and odd-size cases of the GPU test are for."""
  for name in ('b2_t5_24x40_61x103', 'b1_t3_6x9_19x30', 'b1_t2_5x33_17x129'):
    assert (_values(name, True, 'reflect') == _values(name, True)).all()


def test_symbol_and_constants():
  assert 'ra_instance_eval_counts_f32' in rn.SIGNATURES and hasattr(rn.lib(), 'ra_instance_eval_counts_f32')
  assert rn.RA_INS_EVAL_MAX_K == ops.INS_EVAL_MAX_K == 16 and ops.INS_EVAL_MAX_PIXELS == 1 << 24


def test_argument_validation_without_a_device():
  z = torch.zeros
  i32 = lambda *s: torch.zeros(*s, dtype=torch.int32)
  args = (z(1, 2, 4, 4), i32(1, 8, 8), i32(1, 2))
  with pytest.raises(rn.RecAttendError, match='17 thresholds'):
    ops.instance_eval_counts(*args, [0.1] * 17)
  with pytest.raises(rn.RecAttendError, match='0 thresholds'):
    ops.instance_eval_counts(*args, [])
  with pytest.raises(rn.RecAttendError, match='>= 0'):
    ops.instance_eval_counts(*args, [0.3, -0.1])
  with pytest.raises(rn.RecAttendError, match='CPU tensor'):
    ops.instance_eval_counts(*args, [0.3])
  with pytest.raises(rn.RecAttendError, match='CPU tensor'):
    ops.eval_metrics_from_counts(i32(1, 1, 2, 3), i32(1, 2), z(1, 2))
  # the C entry point refuses before any launch, too
  lib = rn.lib()
  buf = np.zeros(64, np.float32)
  p = buf.ctypes.data
  neg = np.array([0.3, -0.1], np.float32)
  call = lambda **kw: lib.ra_instance_eval_counts_f32(*[kw.get(k, d) for k, d in (
      ('yc', p), ('gt_ids', p), ('inst_id', p), ('fg', None), ('B', 1), ('T', 2), ('Hs', 2), ('Ws', 2), ('Hf', 4), ('Wf', 4),
      ('morph', 0), ('thr', p), ('K', 1), ('inter', p), ('area_b', p), ('stream', None))])
  assert call(K=17) == rn.RA_E_SHAPE and call(K=0) == rn.RA_E_SHAPE
  assert call(T=33) == rn.RA_E_SHAPE and call(T=0) == rn.RA_E_SHAPE
  assert call(thr=neg.ctypes.data, K=2) == rn.RA_E_SHAPE
  assert b'threshold 1' in lib.ra_last_error_string()
  assert call(Hf=4097, Wf=4096) == rn.RA_E_SHAPE  # one row over 2^24 pixels
  assert call(gt_ids=None) == rn.RA_E_INVALID and call(inter=None) == rn.RA_E_INVALID and call(Hf=0) == rn.RA_E_INVALID


def _id_archive(tmp_path, **extra):
  path = str(tmp_path / 'ids.npz')
  np.savez(path, x=np.zeros((1, 8, 8, 3), np.float32), gt_instance_ids=np.zeros((1, 12, 10), np.int32), **extra)
  return path


@pytest.mark.parametrize('flag', ['--render', '--render_gt_instances', '--fused_postprocess'])
def test_cli_refuses_by_name_what_the_id_path_cannot_do(tmp_path, flag):
  import full_model_eval
  with pytest.raises(rn.RecAttendError, match=flag + ' cannot be used with an --input that holds gt_instance_ids and no y_gt'):
    full_model_eval.main(['--model_id', 'none', '--results', str(tmp_path), '--input', _id_archive(tmp_path), flag])


def test_cli_keeps_the_plane_path_when_y_gt_is_there(tmp_path):
  import full_model_eval
  assert full_model_eval._id_path(['x', 'gt_instance_ids']) and not full_model_eval._id_path(['x', 'gt_instance_ids', 'y_gt'])
  assert not full_model_eval._id_path(['x', 'y_gt', 's_gt'])
  # with y_gt in the archive --render is today's check (s_gt is missing), not the id path's refusal
  path = _id_archive(tmp_path, y_gt=np.zeros((1, 1, 12, 10), np.float32))
  with pytest.raises(rn.RecAttendError, match='lacks s_gt'):
    full_model_eval.main(['--model_id', 'none', '--results', str(tmp_path), '--input', path, '--render'])


def test_cli_checks_the_id_labels_on_the_host(tmp_path):
  import full_model_eval

  class Args(object):
    input, dataset = 'a.npz', 'cvppp'
  x, ids = np.zeros((2, 8, 8, 3), np.float32), np.zeros((2, 12, 10), np.int32)
  fg = np.zeros((2, 12, 10), np.uint8)
  full_model_eval._check_id_labels(Args, {'x': x, 'gt_instance_ids': ids, 'fg': fg}, None)
  fg[1, 3, 3] = 2
  with pytest.raises(rn.RecAttendError, match='fg of image second holds values other than 0 and 1'):
    full_model_eval._check_id_labels(Args, {'x': x, 'gt_instance_ids': ids, 'fg': fg, 'names': np.array(['first', 'second'])}, None)
  with pytest.raises(rn.RecAttendError, match='fg must be a 0 / 1 mask'):
    full_model_eval._check_id_labels(Args, {'x': x, 'gt_instance_ids': ids, 'fg': fg[:, :8, :8]}, None)
  with pytest.raises(rn.RecAttendError, match='gt_instance_ids must be integers'):
    full_model_eval._check_id_labels(Args, {'x': x, 'gt_instance_ids': ids[:1]}, None)
