"""Pictures on the evaluator's id path on the MI355X: the winner map of ra_instance_eval_counts_map_f32 /
ra_instance_eval_counts_map_ragged_f32 against the float64 oracle (tests/ins_render_oracle.py over ins_eval_oracle) by that
module's band rule, against the counts of the same call (exactly: the map's histogram IS inter) and on exact ties; the paint
kernels (ra_instance_paint_u8, ra_gt_paint_u8 and their ragged forms) byte for byte against the NumPy restatements and, where
the plane chain can run, against ops.render_instances on the chain's masks; the ragged forms against the uniform ones image by
image, gaps untouched; independence from what the outputs held; the refusals.

Bars.  Map: DELTA = 1e-5 and BAND_SHARE = 1e-3 are ins_eval_oracle's constants; tests/test_ins_eval.py holds every case used here
to share <= 1e-3 and zero exact ties on the CPU, so a decided pixel's word is exact and an undecided one lies among its
candidates; where the band is empty (EMPTY_BAND at K = 1, 10 and every edge case) the whole map is equal.  Everything else is an
integer lookup: equal, no tolerance."""
import functools

import numpy as np
import pytest
import torch

import ins_eval_oracle as ieo
import ins_render_oracle as iro
import ra_native as rn
import ra_ops as ops
import ragged_cases as rc
from utils import postprocess as pp

pytestmark = pytest.mark.gpu


def _dev(a, dtype=None):
  return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


@functools.lru_cache(maxsize=None)
def _case(name):
  return ieo.make_case(name)


@functools.lru_cache(maxsize=None)
def _values(name, morph):
  Hf, Wf = ieo.CASES[name][4:6]
  return ieo.values(_case(name)['yc'], Hf, Wf, morph)


def _counts(c, thresholds, fg, morph, **kw):
  return ops.instance_eval_counts(_dev(c['yc']), _dev(c['gt_ids']), _dev(c['inst_id']), thresholds,
                                  fg=None if fg is None else _dev(fg), morph=morph, **kw)


def _np16(t):
  return t.cpu().numpy().astype(np.uint16)


def _misaligned(shape, dtype, by, fill=0):
  """A contiguous device tensor of `shape` whose first element lies `by` elements behind an aligned allocation."""
  n = int(np.prod(shape))
  base = torch.zeros((n + by,), dtype=torch.int16 if dtype == torch.uint16 else dtype, device='cuda')
  base.fill_(fill)
  return base.view(dtype)[by:].view(*shape)


@pytest.mark.parametrize('name', sorted(ieo.CASES))
@pytest.mark.parametrize('morph', [False, True])
@pytest.mark.parametrize('with_fg', [False, True])
def test_map_against_the_oracle_and_the_counts(cuda, name, morph, with_fg):
  c, v = _case(name), _values(name, morph)
  fg = c['fg'] if with_fg else None
  for K in (1, 10, 16):
    thresholds = ieo.THRESHOLDS[K]
    plain = _counts(c, thresholds, fg, morph)
    inter, area_b, wmap = _counts(c, thresholds, fg, morph, want_map=True)
    assert wmap.dtype == torch.uint16 and tuple(wmap.shape) == c['gt_ids'].shape
    assert torch.equal(inter, plain[0]) and torch.equal(area_b, plain[1])  # the same bits with and without the map
    got = _np16(wmap)
    undecided = iro.check_map_in_band(got, v, thresholds, fg)
    print('%s morph %d fg %d K %2d: %d undecided pixels of %d; map == float64 map: %s' % (
        name, morph, with_fg, K, undecided, got.size, bool((got == iro.map_of(v, thresholds, fg)).all())))
    if (name in ieo.EMPTY_BAND and K in (1, 10)) or name in ieo.EDGE_CASES:
      assert (got == iro.map_of(v, thresholds, fg)).all()
    assert ((got >> 8 == 0) == (got == 0)).all()
    # no band here: the map's histogram joined with the slots is inter of the same call
    pos = ops.ins_eval_threshold_pos(thresholds)
    assert (iro.inter_of_map(got, c['gt_ids'], c['inst_id'], pos) == inter.cpu().numpy()).all()
  # element stores (a map that is not 8-byte aligned) write the same words
  out = _misaligned(c['gt_ids'].shape, torch.uint16, 1)
  assert _counts(c, thresholds, fg, morph, map_out=out)[2] is out and (_np16(out) == _np16(wmap)).all()


def test_first_maximum_on_exact_ties(cuda):
  c = dict(_case('b1_t3_16x16_16x16'))
  c['yc'] = c['yc'].copy()
  c['yc'][:, 2] = c['yc'][:, 0]
  for morph in (False, True):
    v = ieo.values(c['yc'], 16, 16, morph)
    for K in (1, 10):
      got = _np16(_counts(c, ieo.THRESHOLDS[K], None, morph, want_map=True)[2])
      assert ((got & 255) != 2).all() and (got == iro.map_of(v, ieo.THRESHOLDS[K])).all()


@pytest.mark.parametrize('name', sorted(ieo.CASES))
def test_paint_and_gt_paint_equal_the_restatements(cuda, name):
  c = _case(name)
  B, T = c['inst_id'].shape
  Hf, Wf = c['gt_ids'].shape[1:]
  for K, with_fg in ((1, False), (10, True), (16, True)):
    thresholds = ieo.THRESHOLDS[K]
    fg = c['fg'] if with_fg else None
    inter, _, wmap = _counts(c, thresholds, fg, with_fg, want_map=True)
    got_map, pos = _np16(wmap), ops.ins_eval_threshold_pos(thresholds)
    colour = iro.random_colours(7 + K, B, K, T)
    keep = (inter.sum(dim=3) > int(inter.sum(dim=3).float().median())).cpu().numpy()  # [B,K,T]: some rows go
    for col, kp, ref_col in ((_dev(colour), None, colour), (_dev(colour), _dev(keep), colour * keep[..., None].astype(np.uint8)),
                             (_dev(colour[0, 0]), None, np.broadcast_to(colour[0, 0], colour.shape)),
                             (None, None, np.broadcast_to(iro.default_colours(32), (B, K, 32, 3)))):
      ref = iro.paint(got_map, pos, ref_col)
      got = ops.paint_instances(wmap, thresholds, colours=col, keep=kp)
      assert tuple(got.shape) == (K, B, Hf, Wf, 3) and (got.cpu().numpy() == ref).all()
      out = _misaligned((K, B, Hf, Wf, 3), torch.uint8, 1, fill=0x5A)  # byte stores
      assert (ops.paint_instances(wmap, thresholds, colours=col, keep=kp, out=out).cpu().numpy() == ref).all()
    moved = _misaligned(wmap.shape, torch.uint16, 1)  # element loads of the map
    moved.view(torch.int16).copy_(wmap.view(torch.int16))
    assert torch.equal(ops.paint_instances(moved, thresholds, colours=_dev(colour)), ops.paint_instances(wmap, thresholds, colours=_dev(colour)))
  gcol = iro.random_colours(3, B, T)
  ref = iro.paint_gt(c['gt_ids'], c['inst_id'], gcol)
  ids, inst = _dev(c['gt_ids']), _dev(c['inst_id'])
  assert (ops.paint_groundtruth(ids, inst, _dev(gcol)).cpu().numpy() == ref).all()
  out = _misaligned((B, Hf, Wf, 3), torch.uint8, 3, fill=0x5A)
  assert (ops.paint_groundtruth(ids, inst, _dev(gcol), out=out).cpu().numpy() == ref).all()
  moved = _misaligned(ids.shape, torch.int32, 1)
  moved.copy_(ids)
  assert (ops.paint_groundtruth(moved, inst, _dev(gcol)).cpu().numpy() == ref).all()
  assert (ops.paint_groundtruth(ids, inst, _dev(gcol[0])).cpu().numpy() == iro.paint_gt(c['gt_ids'], c['inst_id'], np.broadcast_to(gcol[0], gcol.shape))).all()
  neg = c['gt_ids'].copy()
  neg[:, :, ::2] = -1
  assert (ops.paint_groundtruth(_dev(neg), inst, _dev(gcol)).cpu().numpy() == iro.paint_gt(neg, c['inst_id'], gcol)).all()


def test_default_palette_wraps_at_t32(cuda):
  name = 'b1_t32_12x20_40x132'
  c = _case(name)
  inter, _, wmap = _counts(c, [0.3], None, False, want_map=True)
  got_map = _np16(wmap)
  assert ((got_map & 255)[got_map > 0] >= 22).any()
  tab = iro.default_colours(32)
  ref = iro.paint(got_map, [0], tab[None, None])
  assert (ops.paint_instances(wmap, [0.3]).cpu().numpy() == ref).all()
  assert (ref[0, 0][(got_map[0] & 255) >= 22].max(axis=-1) > 0).all()  # the wrapped rows are colours, not black
  assert (ops.paint_instances(wmap, [0.3], keep=_dev(np.ones((1, 1, 32), bool))).cpu().numpy() == ref).all()


def test_pictures_equal_the_render_stage_on_the_plane_chain(cuda):
  """b2_t4_10x14_36x52 (empty band, Hf * Wf % 4 == 0) with fg + morph + remove_tiny: what the parent commit's route gives —
  ops.render_instances on the chain's masks — is what the map gives."""
  name = 'b2_t4_10x14_36x52'
  c = _case(name)
  thresholds = ieo.THRESHOLDS[10]
  fgd = _dev(c['fg'], np.float32)
  one = pp.apply_one_label(pp.morph(pp.upsample(_dev(c['yc']), (36, 52))))
  inter, area_b, wmap = _counts(c, thresholds, c['fg'], True, want_map=True)
  s_gt = _dev(c['s_gt'])
  areas = inter.sum(dim=3)
  tiny = int(areas[areas > 0].float().median())  # an area that occurs: at least one prediction goes, the larger ones stay
  per = ops.eval_metrics_from_counts(inter, area_b, s_gt, remove_tiny=tiny, conf=torch.ones_like(s_gt))
  keep = ops.paint_keep(per)
  assert keep.dtype == torch.bool and tuple(keep.shape) == (2, 10, 4) and not bool(keep.all()) and bool(keep.any())
  pictures = ops.paint_instances(wmap, thresholds, keep=keep)
  for k, th in enumerate(thresholds):
    y, _ = pp.remove_tiny(pp.mask_foreground(pp.apply_threshold(one, th), fgd), torch.ones_like(s_gt), threshold=tiny)
    assert torch.equal(pictures[k], ops.render_instances(y.contiguous())), th
  gcol = _dev(iro.random_colours(5, 2, 4))
  planes = _dev(ieo.gt_planes(c['gt_ids'], c['inst_id']))
  assert torch.equal(ops.paint_groundtruth(_dev(c['gt_ids']), _dev(c['inst_id']), gcol), ops.render_instances(planes, colours=gcol, first=True))


def _packed(images, name, dtype, fill=0):
  order, align = rc.layout(name, len(images))
  geo, total = rc.geometry([images[i].shape for i in order], align)
  return _dev(rc.flatten([images[i] for i in order], geo, total, dtype, fill)), geo, order, total


@pytest.mark.parametrize('layout', rc.LAYOUTS)
@pytest.mark.parametrize('with_fg', [False, True])
def test_ragged_forms_equal_the_uniform_ones_image_by_image(cuda, layout, with_fg):
  n = len(rc.EVAL_SIZES)
  cases = [rc.ins_eval_image(i) for i in range(n)]
  T = rc.EVAL_T
  morph = with_fg
  gt, geo, order, total = _packed([c['gt_ids'][0] for c in cases], layout, np.int32)
  fg = _packed([c['fg'][0] for c in cases], layout, np.uint8)[0] if with_fg else None
  yc = _dev(np.concatenate([c['yc'] for c in cases])[order])
  inst = _dev(np.concatenate([c['inst_id'] for c in cases])[order])
  inside = np.zeros(total, bool)
  for off, h, w in geo.tolist():
    inside[off:off + h * w] = True
  assert layout != 'aligned' or not inside.all()  # this layout has gaps
  gcol = iro.random_colours(9, n, T)
  for K in (1, 10):
    thr = ieo.THRESHOLDS[K]
    plain = ops.instance_eval_counts_ragged(yc, gt, geo, inst, thr, fg_flat=fg, morph=morph)
    wmap = _misaligned((total,), torch.uint16, 0, fill=0xABAB - 0x10000)
    inter, area_b, back = ops.instance_eval_counts_ragged(yc, gt, geo, inst, thr, fg_flat=fg, morph=morph, map_out=wmap)
    assert back is wmap and torch.equal(inter, plain[0]) and torch.equal(area_b, plain[1])
    colour = iro.random_colours(K, n, K, T)
    pics = torch.full((K, total, 3), 0xAB, dtype=torch.uint8, device='cuda')
    assert ops.paint_instances(wmap, thr, colours=_dev(colour), geo=geo, out=pics) is pics
    gpic = torch.full((total, 3), 0xAB, dtype=torch.uint8, device='cuda')
    ops.paint_groundtruth(gt, inst, _dev(gcol), geo=geo, out=gpic)
    m, p, g = _np16(wmap), pics.cpu().numpy(), gpic.cpu().numpy()
    assert (m[~inside] == 0xABAB).all() and (p[:, ~inside] == 0xAB).all() and (g[~inside] == 0xAB).all()  # the gaps
    for b, (i, (off, h, w)) in enumerate(zip(order, geo.tolist())):
      c = cases[i]
      alone = ops.instance_eval_counts(_dev(c['yc']), _dev(c['gt_ids']), _dev(c['inst_id']), thr, fg=_dev(c['fg']) if with_fg else None,
                                       morph=morph, want_map=True)
      assert torch.equal(alone[0][0], inter[b]) and torch.equal(alone[1][0], area_b[b])
      assert (m[off:off + h * w].reshape(h, w) == _np16(alone[2][0])).all(), (i, K)
      ref = ops.paint_instances(alone[2], thr, colours=_dev(colour[b:b + 1])).cpu().numpy()
      assert (p[:, off:off + h * w].reshape(K, h, w, 3) == ref[:, 0]).all(), (i, K)
      ref = ops.paint_groundtruth(_dev(c['gt_ids']), _dev(c['inst_id']), _dev(gcol[b:b + 1])).cpu().numpy()
      assert (g[off:off + h * w].reshape(h, w, 3) == ref[0]).all(), (i, K)
  # a map and pictures made by the wrappers start as zeros between the images
  made = ops.instance_eval_counts_ragged(yc, gt, geo, inst, thr, fg_flat=fg, morph=morph, want_map=True)[2]
  assert (_np16(made)[~inside] == 0).all() and (_np16(made)[inside] == m[inside]).all()
  assert (ops.paint_instances(made, thr, colours=_dev(colour), geo=geo).cpu().numpy()[:, ~inside] == 0).all()


def test_outputs_do_not_depend_on_what_the_memory_held(cuda):
  c = _case('b2_t4_8x12_37x50')
  thr = ieo.THRESHOLDS[10]
  results = []
  for fill in (0, -1):
    wmap = _misaligned(c['gt_ids'].shape, torch.uint16, 0, fill=fill)
    _counts(c, thr, c['fg'], True, map_out=wmap)
    pics = torch.full((10, 2, 37, 50, 3), fill & 255, dtype=torch.uint8, device='cuda')
    ops.paint_instances(wmap, thr, out=pics)
    gpic = torch.full((2, 37, 50, 3), fill & 255, dtype=torch.uint8, device='cuda')
    ops.paint_groundtruth(_dev(c['gt_ids']), _dev(c['inst_id']), _dev(iro.random_colours(1, 4)), out=gpic)
    results.append((wmap, pics, gpic))
  for a, b in zip(*results):
    assert (a.cpu().numpy() == b.cpu().numpy()).all()


def test_refusals(cuda):
  c = _case('b1_t3_16x16_16x16')
  wmap = _counts(c, [0.3], None, False, want_map=True)[2]
  ids, inst = _dev(c['gt_ids']), _dev(c['inst_id'])
  with pytest.raises(rn.RecAttendError, match='0 thresholds'):
    ops.paint_instances(wmap, [])
  with pytest.raises(rn.RecAttendError, match='17 thresholds'):
    ops.paint_instances(wmap, [0.3] * 17)
  with pytest.raises(rn.RecAttendError, match='T=33'):
    ops.paint_instances(wmap, [0.3], colours=torch.zeros(33, 3, dtype=torch.uint8, device='cuda'))
  with pytest.raises(rn.RecAttendError, match=r'inst_id must be \[B,T\]'):
    ops.paint_groundtruth(ids, torch.zeros(1, 33, dtype=torch.int32, device='cuda'), torch.zeros(33, 3, dtype=torch.uint8, device='cuda'))
  with pytest.raises(rn.RecAttendError, match='map must be contiguous torch.uint16'):
    ops.paint_instances(wmap.view(torch.int16), [0.3])
  with pytest.raises(rn.RecAttendError, match='map_out must be contiguous uint16'):
    _counts(c, [0.3], None, False, map_out=torch.zeros(1, 16, 16, dtype=torch.int16, device='cuda'))
  with pytest.raises(rn.RecAttendError, match='map_out must be contiguous uint16'):
    _counts(c, [0.3], None, False, map_out=torch.zeros(1, 16, 15, dtype=torch.uint16, device='cuda'))
  with pytest.raises(rn.RecAttendError, match='keep must be a bool device tensor'):
    ops.paint_instances(wmap, [0.3], keep=torch.ones(1, 2, 3, dtype=torch.bool, device='cuda'))
  with pytest.raises(rn.RecAttendError, match='colours must be'):
    ops.paint_instances(wmap, [0.3], colours=torch.zeros(2, 1, 3, 3, dtype=torch.uint8, device='cuda'))
  with pytest.raises(rn.RecAttendError, match='out must be a contiguous uint8 device tensor'):
    ops.paint_instances(wmap, [0.3], out=torch.zeros(1, 1, 16, 16, 4, dtype=torch.uint8, device='cuda'))
  # the ragged forms: a flat map of another length than the geometry's tensors, and a table whose entries overlap
  flat = wmap.view(-1)
  geo = np.array([[0, 8, 16], [200, 8, 16]], np.int64)  # image 1 ends beyond the 256 elements
  with pytest.raises(rn.RecAttendError, match='image 1 .* beyond the buffer'):
    ops.paint_instances(flat, [0.3], geo=geo)
  over = np.array([[0, 8, 16], [64, 8, 16]], np.int64)
  for call in (lambda: ops.paint_instances(flat, [0.3], geo=over),
               lambda: ops.paint_groundtruth(ids.view(-1), inst.expand(2, 3).contiguous(), torch.ones(3, 3, dtype=torch.uint8, device='cuda'), geo=over),
               lambda: ops.instance_eval_counts_ragged(_dev(np.repeat(c['yc'], 2, 0)), ids.view(-1), over, inst.expand(2, 3).contiguous(), [0.3],
                                                       want_map=True)):
    with pytest.raises(rn.RecAttendError, match='image 1 starts at element 64, inside image 0'):
      call()
  with pytest.raises(rn.RecAttendError, match='map_out must be contiguous uint16'):
    ops.instance_eval_counts_ragged(_dev(c['yc']), ids.view(-1), np.array([[0, 16, 16]]), inst, [0.3],
                                    map_out=torch.zeros(255, dtype=torch.uint16, device='cuda'))
  with pytest.raises(rn.RecAttendError, match='with a geometry map must be flat'):
    ops.paint_instances(wmap, [0.3], geo=np.array([[0, 16, 16]]))
  # the C entry point on device memory: nothing is launched and the output keeps what it held
  out = torch.full((1, 16, 16, 3), 7, dtype=torch.uint8, device='cuda')
  pos = np.zeros(1, np.int32)
  col = torch.zeros(1, 17, 3, 3, dtype=torch.uint8, device='cuda')
  rcode = rn.lib().ra_instance_paint_u8(wmap.data_ptr(), 1, 16, 16, pos.ctypes.data, 17, 3, col.data_ptr(), out.data_ptr(), rn.stream_ptr())
  torch.cuda.synchronize()
  assert rcode == rn.RA_E_SHAPE and int(out.min()) == 7
