"""Pictures on the evaluator's id path, without a device: the winner map and the paint rules of tests/ins_render_oracle.py
against the reference's own composition from the chain's masks (analysis.py:137-147 on ins_eval_oracle.masks), the ground
truth's picture against first-mode composition of ins_eval_oracle.gt_planes, a named case per mutant of a rule, the symbols,
the host-side refusals of the C entry points and the wrappers, and the command line's refusal of the two new flags where the
id path does not run."""
import functools

import numpy as np
import pytest
import torch

import ins_eval_oracle as ieo
import ins_render_oracle as iro
import ra_native as rn
import ra_ops as ops

ROUTE_CASES = ['b2_t5_24x40_61x103', 'b1_t3_16x16_16x16', 'b3_t2_4x4_2x3', 'b1_t1_1x1_1x4']  # test_counts_route_equals_masks_route's
SYMBOLS = ('ra_instance_eval_counts_map_f32', 'ra_instance_eval_counts_map_ragged_f32', 'ra_instance_eval_threshold_pos',
           'ra_instance_paint_u8', 'ra_instance_paint_ragged_u8', 'ra_gt_paint_u8', 'ra_gt_paint_ragged_u8')


@functools.lru_cache(maxsize=None)
def _case(name):
  return ieo.make_case(name)


@functools.lru_cache(maxsize=None)
def _values(name, morph):
  Hf, Wf = ieo.CASES[name][4:6]
  return ieo.values(_case(name)['yc'], Hf, Wf, morph)


def _pictures_from_masks(v, thresholds, fg, colour, keep=None):
  """[K,B,Hf,Wf,3]: the reference's formula on the chain's masks, the planes remove_tiny took zeroed."""
  out = []
  for k, th in enumerate(thresholds):
    y = ieo.masks(v, th, fg)
    if keep is not None:
      y = y * keep[:, k][:, :, None, None]
    out.append(iro.picture_from_masks(y, colour[:, k]))
  return np.stack(out)


@pytest.mark.parametrize('name', ROUTE_CASES)
@pytest.mark.parametrize('morph', [False, True])
@pytest.mark.parametrize('with_fg', [False, True])
@pytest.mark.parametrize('K', [1, 10, 16])
def test_painted_map_equals_the_pictures_composed_from_masks(name, morph, with_fg, K):
  c, v = _case(name), _values(name, morph)
  fg = c['fg'] if with_fg else None
  B, T = c['inst_id'].shape
  thresholds = ieo.THRESHOLDS[K]  # K = 16 repeats 0.3
  colour = iro.random_colours(7, B, K, T)
  wmap, pos = iro.map_of(v, thresholds, fg), iro.threshold_pos(thresholds)
  assert wmap.dtype == np.uint16 and ((wmap >> 8 == 0) == (wmap == 0)).all()
  assert (iro.paint(wmap, pos, colour) == _pictures_from_masks(v, thresholds, fg, colour)).all()
  # remove_tiny on the counted areas: a zeroed colour row
  inter, _ = ieo.counts(v, c['gt_ids'], c['inst_id'], thresholds, fg)
  tiny = int(np.median(inter.sum(axis=3)))
  keep = iro.keep_of(v, c['gt_ids'], c['inst_id'], thresholds, fg, tiny)
  got = iro.paint(wmap, pos, colour * keep[..., None].astype(np.uint8))
  assert (got == _pictures_from_masks(v, thresholds, fg, colour, keep)).all()
  # ... and the map's histogram is the counts
  assert (iro.inter_of_map(wmap, c['gt_ids'], c['inst_id'], pos) == inter).all()


@pytest.mark.parametrize('name', sorted(ieo.CASES))
def test_gt_paint_equals_first_mode_composition_of_the_planes(name):
  c = _case(name)
  B, T = c['inst_id'].shape
  colour = iro.random_colours(11, B, T)
  planes = ieo.gt_planes(c['gt_ids'], c['inst_id'])
  got = iro.paint_gt(c['gt_ids'], c['inst_id'], colour)
  assert (got == iro.picture_first(planes, colour)).all()
  assert (got == iro.picture_from_masks(planes, colour)).all()  # disjoint planes: adding is laying under
  neg = c['gt_ids'].copy()
  neg[:, ::2] = -1  # an empty slot's -1 matches no pixel
  assert (iro.paint_gt(neg, c['inst_id'], colour)[:, ::2] == 0).all()


def test_mutant_ge_in_the_pos_rule_is_rejected():
  """n >= pos[k] in place of n > pos[k]: at the lowest threshold pos is 0, and every pixel nobody holds (n = 0) gets colour."""
  name = 'b2_t4_8x12_37x50'
  c, v = _case(name), _values(name, False)
  thresholds = ieo.THRESHOLDS[10]
  colour = iro.random_colours(7, 2, 10, 4)
  wmap, pos = iro.map_of(v, thresholds, c['fg']), iro.threshold_pos(thresholds)
  ref = _pictures_from_masks(v, thresholds, c['fg'], colour)
  assert (iro.paint(wmap, pos, colour) == ref).all()
  assert (iro.paint(wmap, pos, colour, mutant='ge') != ref).any()


def test_mutant_last_maximum_is_rejected_on_exact_ties():
  c = dict(_case('b1_t3_16x16_16x16'))
  c['yc'] = c['yc'].copy()
  c['yc'][:, 2] = c['yc'][:, 0]
  v = ieo.values(c['yc'], 16, 16, False)
  thresholds = ieo.THRESHOLDS[10]
  colour = iro.random_colours(7, 1, 10, 3)
  pos = iro.threshold_pos(thresholds)
  ref = _pictures_from_masks(v, thresholds, None, colour)
  first, last = iro.map_of(v, thresholds), iro.map_of(v, thresholds, mutant='last_max')
  assert ((first & 255) != 2).all() and ((last & 255) == 2).any()
  assert (iro.paint(first, pos, colour) == ref).all()
  assert (iro.paint(last, pos, colour) != ref).any()


def test_mutant_palette_without_wrap_is_rejected_at_t32():
  """The default palette is INSTANCE_CMAP[t % 22]: predictions 22 .. 31 take the colours of 0 .. 9, not black and not a row
  beyond the table."""
  tab = iro.default_colours(32)
  assert tab.shape == (32, 3) and (tab[22:] == tab[:10]).all() and (tab.reshape(32, -1).max(axis=1) > 0).all()
  name = 'b1_t32_12x20_40x132'
  c, v = _case(name), _values(name, False)
  wmap, pos = iro.map_of(v, [0.3]), iro.threshold_pos([0.3])
  assert ((wmap & 255)[wmap > 0] >= 22).any()  # the case does reach the wrapped rows
  ref = _pictures_from_masks(v, [0.3], None, tab[None, None])
  assert (iro.paint(wmap, pos, tab[None, None]) == ref).all()
  clipped = tab.copy()
  clipped[22:] = 0
  assert (iro.paint(wmap, pos, clipped[None, None]) != ref).any()


def test_threshold_pos_is_the_counting_pass_s_order():
  for K in (1, 10, 16):
    assert (ops.ins_eval_threshold_pos(ieo.THRESHOLDS[K]) == iro.threshold_pos(np.float32(ieo.THRESHOLDS[K]))).all()
  assert ops.ins_eval_threshold_pos([0.5, 0.1, 0.5, 0.3]).tolist() == [2, 0, 2, 1]
  with pytest.raises(rn.RecAttendError, match='17 thresholds'):
    ops.ins_eval_threshold_pos([0.1] * 17)
  with pytest.raises(rn.RecAttendError, match='0 thresholds'):
    ops.ins_eval_threshold_pos([])
  with pytest.raises(rn.RecAttendError, match='>= 0'):
    ops.ins_eval_threshold_pos([-0.1])


def test_symbols_in_header_and_binding():
  I, P, Z = rn.C.c_int, rn.C.c_void_p, rn.C.c_size_t
  for s in SYMBOLS:
    assert s in rn.SIGNATURES and hasattr(rn.lib(), s), s
  assert rn.SIGNATURES['ra_instance_eval_counts_map_f32'] == (I, rn.SIGNATURES['ra_instance_eval_counts_f32'][1][:-1] + [P, P])
  assert rn.SIGNATURES['ra_instance_eval_counts_map_ragged_f32'] == (
      I, rn.SIGNATURES['ra_instance_eval_counts_ragged_f32'][1][:-1] + [P, P])
  assert rn.SIGNATURES['ra_instance_paint_u8'] == (I, [P, I, I, I, P, I, I, P, P, P])
  assert rn.SIGNATURES['ra_instance_paint_ragged_u8'] == (I, [P, Z, P, P, I, P, I, I, P, P, P])
  assert rn.SIGNATURES['ra_gt_paint_u8'] == (I, [P, P, I, I, I, I, P, P, P])
  assert rn.SIGNATURES['ra_gt_paint_ragged_u8'] == (I, [P, Z, P, P, P, I, I, P, P, P])


def test_c_entry_points_refuse_on_the_host():
  lib = rn.lib()
  buf = np.zeros(256, np.int32)
  p = buf.ctypes.data
  pos = np.zeros(17, np.int32)
  paint = lambda **kw: lib.ra_instance_paint_u8(*[kw.get(k, d) for k, d in (
      ('map', p), ('B', 1), ('Hf', 4), ('Wf', 4), ('pos', pos.ctypes.data), ('Kp', 1), ('T', 2), ('colour', p), ('out', p), ('stream', None))])
  assert paint(Kp=0) == rn.RA_E_SHAPE and paint(Kp=17) == rn.RA_E_SHAPE and b'Kp=17' in lib.ra_last_error_string()
  assert paint(T=33) == rn.RA_E_SHAPE and b'T=33' in lib.ra_last_error_string() and paint(T=0) == rn.RA_E_SHAPE
  assert paint(Hf=4097, Wf=4096) == rn.RA_E_SHAPE
  assert paint(map=None) == rn.RA_E_INVALID and paint(out=None) == rn.RA_E_INVALID and paint(Hf=0) == rn.RA_E_INVALID
  bad = np.array([16], np.int32)
  assert paint(pos=bad.ctypes.data) == rn.RA_E_SHAPE and b'pos[0] = 16' in lib.ra_last_error_string()
  gt = lambda **kw: lib.ra_gt_paint_u8(*[kw.get(k, d) for k, d in (
      ('gt_ids', p), ('inst_id', p), ('B', 1), ('T', 2), ('Hf', 4), ('Wf', 4), ('colour', p), ('out', p), ('stream', None))])
  assert gt(T=33) == rn.RA_E_SHAPE and gt(T=0) == rn.RA_E_SHAPE and gt(B=65536) == rn.RA_E_SHAPE
  assert gt(inst_id=None) == rn.RA_E_INVALID and gt(Wf=0) == rn.RA_E_INVALID
  # the ragged forms check the table before anything else touches the device, and name the image
  tab = (rn.ImageGeo * 2)(rn.ImageGeo(0, 4, 4), rn.ImageGeo(8, 4, 4))
  rcode = lib.ra_instance_paint_ragged_u8(p, 64, tab, p, 2, pos.ctypes.data, 1, 2, p, p, None)
  assert rcode == rn.RA_E_SHAPE and b'image 1 starts at element 8, inside image 0' in lib.ra_last_error_string()
  rcode = lib.ra_gt_paint_ragged_u8(p, 24, (rn.ImageGeo * 2)(rn.ImageGeo(0, 4, 4), rn.ImageGeo(16, 4, 4)), p, p, 2, 2, p, p, None)
  assert rcode == rn.RA_E_SHAPE and b'image 1' in lib.ra_last_error_string() and b'beyond the buffer' in lib.ra_last_error_string()
  assert lib.ra_instance_paint_ragged_u8(p, 64, tab, p, 2, pos.ctypes.data, 17, 2, p, p, None) == rn.RA_E_SHAPE
  # the map forms of the counting pass: the checks of the plain forms, and a map is required
  thr = np.array([0.3], np.float32)
  call = lambda **kw: lib.ra_instance_eval_counts_map_f32(*[kw.get(k, d) for k, d in (
      ('yc', p), ('gt_ids', p), ('inst_id', p), ('fg', None), ('B', 1), ('T', 2), ('Hs', 2), ('Ws', 2), ('Hf', 4), ('Wf', 4),
      ('morph', 0), ('thr', thr.ctypes.data), ('K', 1), ('inter', p), ('area_b', p), ('map', p), ('stream', None))])
  assert call(map=None) == rn.RA_E_INVALID and call(K=17) == rn.RA_E_SHAPE and call(T=33) == rn.RA_E_SHAPE
  assert b'ra_instance_eval_counts_map_f32' in lib.ra_last_error_string()
  assert lib.ra_instance_eval_counts_map_ragged_f32(p, p, p, None, 64, tab, p, 2, 2, 2, 2, 0, thr.ctypes.data, 1, p, p, None, None) == rn.RA_E_INVALID
  assert lib.ra_instance_eval_counts_map_ragged_f32(p, p, p, None, 64, tab, p, 2, 2, 2, 2, 0, thr.ctypes.data, 1, p, p, p, None) == rn.RA_E_SHAPE
  assert b'image 1 starts at element 8' in lib.ra_last_error_string()


def test_wrappers_refuse_without_a_device():
  u16 = lambda *s: torch.zeros(*s, dtype=torch.uint16)
  i32 = lambda *s: torch.zeros(*s, dtype=torch.int32)
  u8 = lambda *s: torch.zeros(*s, dtype=torch.uint8)
  with pytest.raises(rn.RecAttendError, match='CPU tensor'):
    ops.paint_instances(u16(1, 4, 4), [0.3])
  with pytest.raises(rn.RecAttendError, match='17 thresholds'):
    ops.paint_instances(u16(1, 4, 4), [0.3] * 17)
  with pytest.raises(rn.RecAttendError, match='0 thresholds'):
    ops.paint_instances(u16(1, 4, 4), [])
  with pytest.raises(rn.RecAttendError, match='CPU tensor'):
    ops.paint_groundtruth(i32(1, 4, 4), i32(1, 2), u8(2, 3))
  with pytest.raises(rn.RecAttendError, match='CPU tensor'):
    ops.instance_eval_counts(torch.zeros(1, 2, 4, 4), i32(1, 8, 8), i32(1, 2), [0.3], want_map=True)
  with pytest.raises(rn.RecAttendError, match='CPU tensor'):
    ops.instance_eval_counts_ragged(torch.zeros(1, 2, 4, 4), i32(64), np.array([[0, 8, 8]]), i32(1, 2), [0.3], want_map=True)


def _archive(tmp_path, **arrays):
  path = str(tmp_path / 'in.npz')
  np.savez(path, x=np.zeros((1, 8, 8, 3), np.float32), **arrays)
  return path


@pytest.mark.parametrize('flag', ['--render_from_ids', '--render_gt_from_ids'])
def test_cli_refuses_the_new_flags_by_name_off_the_id_path(tmp_path, flag):
  import full_model_eval
  ids, planes = np.zeros((1, 12, 10), np.int32), np.zeros((1, 1, 12, 10), np.float32)
  other = {'--render_from_ids': '--render', '--render_gt_from_ids': '--render_gt_instances'}[flag]
  for arrays in (dict(y_gt=planes, s_gt=np.zeros((1, 1), np.float32)), dict(y_gt=planes, gt_instance_ids=ids), {}):
    with pytest.raises(rn.RecAttendError, match=flag + ' cannot be used with an --input that takes the plane path') as e:
      full_model_eval.main(['--model_id', 'none', '--results', str(tmp_path), '--input', _archive(tmp_path, **arrays), flag])
    assert other in str(e.value)
  with pytest.raises(rn.RecAttendError, match=flag + ' needs --input with gt_instance_ids') as e:
    full_model_eval.main(['--model_id', 'none', '--results', str(tmp_path), flag])
  assert other in str(e.value)
