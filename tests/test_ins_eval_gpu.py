"""The evaluator from instance-id images on the MI355X: ra_instance_eval_counts_f32 (ops.instance_eval_counts) against the
float64 oracle of tests/ins_eval_oracle.py by its band rule — equal to the oracle's counts wherever the band is empty, area_b
always equal — with the plane kernels' chain of utils/postprocess.py held to the same band, the metrics from the counts
(ops.eval_metrics_from_counts) against ops.eval_metrics on the chain's masks and against the float64 oracle, the refusals, and
full_model_eval.py end to end on an archive of id images.

Bars.  Counts: the band of ins_eval_oracle (DELTA = 1e-5, at most 0.1 % undecided pixels per image and threshold, no exact
ties: conditions on the inputs, asserted here too).  Metrics: eval_cases.TOL_METRICS = 1e-6 against float64 arithmetic on the
device's own integers; element for element against ops.eval_metrics, which runs the same kernel on the same float inputs.
The chain's plane kernels need Hf * Wf % 4 == 0 (ra_postprocess_f32, ra_pair_stats_f32), so the chain is run on the cases
that have it.  The output holds exactly K thresholds' slots ([B,K,T,T + 1]), so there are no unused slots to stay zero; what
is checked in their place is that a repeated threshold gets the same counts twice and that the result does not depend on what
the output memory held before."""
import functools
import os

import numpy as np
import pytest
import torch

import eval_cases
import ins_eval_oracle as ieo
import ra_native as rn
import ra_ops as ops
import ra_oracle as ora
from utils import postprocess as pp

pytestmark = pytest.mark.gpu
TOL_METRICS = eval_cases.TOL_METRICS
STAT_CHECKED = ('sbd', 'wt_cov', 'unwt_cov', 'fg_iou', 'fg_dice', 'avg_fp', 'avg_fn', 'count_acc', 'count_mse', 'dic', 'dic_abs')


def _dev(a, dtype=None):
  return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


@functools.lru_cache(maxsize=None)
def _case(name):
  return ieo.make_case(name)


@functools.lru_cache(maxsize=None)
def _values(name, morph):
  Hf, Wf = ieo.CASES[name][4:6]
  return ieo.values(_case(name)['yc'], Hf, Wf, morph)


def _fused(c, thresholds, fg, morph):
  inter, area_b = ops.instance_eval_counts(_dev(c['yc']), _dev(c['gt_ids']), _dev(c['inst_id']), thresholds,
                                           fg=None if fg is None else _dev(fg), morph=morph)
  return inter, area_b


def _chain_masks(c, thresholds, fg, morph):
  """The parent commit's device chain behind apply_confidence: one [B,T,Hf,Wf] tensor of binary masks per threshold."""
  Hf, Wf = c['gt_ids'].shape[1:]
  v = pp.upsample(_dev(c['yc']), (Hf, Wf))
  if morph:
    v = pp.morph(v)
  one = pp.apply_one_label(v)
  out = []
  for th in thresholds:
    y = pp.apply_threshold(one, th)
    out.append(y if fg is None else pp.mask_foreground(y, _dev(fg, np.float32)))
  return out


@pytest.mark.parametrize('name', sorted(ieo.CASES))
@pytest.mark.parametrize('morph', [False, True])
@pytest.mark.parametrize('with_fg', [False, True])
def test_counts_against_the_oracle(cuda, name, morph, with_fg):
  c, v = _case(name), _values(name, morph)
  fg = c['fg'] if with_fg else None
  Hf, Wf = c['gt_ids'].shape[1:]
  for K in (1, 10, 16):
    thresholds = ieo.THRESHOLDS[K]
    lo, hi, share, ties = ieo.conditions(v, c['gt_ids'], c['inst_id'], thresholds, fg)
    assert share <= ieo.BAND_SHARE and ties == 0
    ref_inter, ref_area = ieo.counts(v, c['gt_ids'], c['inst_id'], thresholds, fg)
    runs = [_fused(c, thresholds, fg, morph) for _ in range(3)]
    for inter, area_b in runs[1:]:  # integer atomics: the same bits on every run
      assert torch.equal(inter, runs[0][0]) and torch.equal(area_b, runs[0][1])
    inter, area_b = runs[0][0].cpu().numpy().astype(np.int64), runs[0][1].cpu().numpy().astype(np.int64)
    assert inter.shape == ref_inter.shape and area_b.shape == ref_area.shape
    empty = bool((lo == hi).all())
    print('%s morph %d fg %d K %2d: band of %d counts (share %.5f), fused differs from the float64 counts in %d of %d entries' % (
        name, morph, with_fg, K, int((hi - lo).sum()), share, int((inter != ref_inter).sum()), inter.size))
    assert (area_b == ref_area).all()
    assert (lo <= inter).all() and (inter <= hi).all()
    if empty:
      assert (inter == ref_inter).all()
    if K == 16:  # 0.3 is given twice (slots 3 and 4)
      assert (inter[:, 3] == inter[:, 4]).all()
    if (Hf * Wf) % 4 == 0:
      chain = np.stack([ieo.counts_of_masks(y.cpu().numpy(), c['gt_ids'], c['inst_id'])[0] for y in _chain_masks(c, thresholds, fg, morph)],
                       axis=1)
      print('    the chain of plane kernels: fused == chain is %s' % bool((chain == inter).all()))
      assert (lo <= chain).all() and (chain <= hi).all()


def test_first_maximum_on_exact_ties(cuda):
  """Instance 2 is a copy of instance 0: equal inputs give equal values on the device, and the lower index must take the pixel.
  Without the copy the case has an empty band (tests/test_ins_eval.py), so the oracle's counts are the bar."""
  c = dict(_case('b1_t3_16x16_16x16'))
  c['yc'] = c['yc'].copy()
  c['yc'][:, 2] = c['yc'][:, 0]
  for morph in (False, True):
    v = ieo.values(c['yc'], 16, 16, morph)
    for K in (1, 10):
      ref, _ = ieo.counts(v, c['gt_ids'], c['inst_id'], ieo.THRESHOLDS[K])
      got = _fused(c, ieo.THRESHOLDS[K], None, morph)[0].cpu().numpy()
      assert got[:, :, 2].sum() == 0 and (got == ref).all()


def _check_metrics(met, ref, what):
  stats, inst, iou = met['stats'].cpu().numpy(), met['inst'].cpu().numpy(), met['iou_pairwise'].cpu().numpy()
  worst = 0.0
  for n in STAT_CHECKED:
    err = float(np.abs(stats[:, ops.EVAL_NAMES.index(n)] - ref[n]).max())
    worst = max(worst, err)
    assert err <= TOL_METRICS, (what, n, err)
  err = float(np.abs(iou - ref['iou_pairwise']).max())
  assert err <= TOL_METRICS, (what, 'iou_pairwise', err)
  col = lambda n: inst[:, ops.EVALI_NAMES.index(n)]
  for n, key, gate in (('pix_pr', 'avg_pr', 'has_out'), ('obj_pr', 'obj_pr', 'has_out'), ('pix_re', 'avg_re', 'is_gt'),
                       ('obj_re', 'obj_re', 'is_gt')):
    got = col(n)[col(gate) > 0]
    assert got.shape == ref[key].shape, (what, key)
    err = float(np.abs(got - ref[key]).max(initial=0))
    worst = max(worst, err)
    assert err <= TOL_METRICS, (what, key, err)
  print('%s: largest |device - float64| over the metrics %.3g' % (what, max(worst, float(np.abs(iou - ref['iou_pairwise']).max()))))


@pytest.mark.parametrize('name', ['b1_t3_16x16_16x16', 'b2_t4_10x14_36x52', 'b1_t1_1x1_1x4', 'b2_t5_24x40_61x103', 'b1_t32_12x20_40x132'])
@pytest.mark.parametrize('with_fg', [False, True])
def test_metrics_from_counts(cuda, name, with_fg):
  c = _case(name)
  morph, fg = with_fg, (c['fg'] if with_fg else None)  # as the command line runs it: the dilation goes with the foreground
  Hf, Wf = c['gt_ids'].shape[1:]
  thresholds = ieo.THRESHOLDS[10]
  inter, area_b = _fused(c, thresholds, fg, morph)
  s_gt = _dev(c['s_gt'])
  per = ops.eval_metrics_from_counts(inter, area_b, s_gt)
  assert len(per) == len(thresholds)
  cnt, area = inter.cpu().numpy().astype(np.int64), area_b.cpu().numpy().astype(np.int64)
  for k, th in enumerate(thresholds):  # float64 arithmetic on the device's own integers
    _check_metrics(per[k], ieo.metrics_from_counts(cnt[:, k], area, c['s_gt'].astype(np.float64)), '%s fg %d thr %.1f' % (name, with_fg, th))
    assert torch.equal(per[k]['sizes'], inter[:, k].sum(dim=2).to(torch.float32))
  lo, hi, _, _ = ieo.conditions(_values(name, morph), c['gt_ids'], c['inst_id'], thresholds, fg)
  if (Hf * Wf) % 4 == 0 and (lo == hi).all():  # same kernel, same float inputs: element for element
    y_gt = _dev(ieo.gt_planes(c['gt_ids'], c['inst_id']))
    for k, y in enumerate(_chain_masks(c, thresholds, fg, morph)):
      ref = ops.eval_metrics(y.contiguous(), y_gt, s_gt)
      for key in ('iou_pairwise', 'stats', 'inst', 'sizes'):
        assert torch.equal(per[k][key], ref[key]), (name, with_fg, thresholds[k], key)
  else:
    assert name not in ('b1_t3_16x16_16x16', 'b2_t4_10x14_36x52', 'b1_t1_1x1_1x4')  # these three must take the branch above


def test_remove_tiny_on_the_counts(cuda):
  """A prediction of area a survives remove_tiny = a - 1 and vanishes, with its confidence, at a and a + 1 (postprocess.py:
  115,131: size > threshold stays); each time the result is the chain's — mask_foreground -> remove_tiny -> ops.eval_metrics —
  element for element."""
  name = 'b2_t4_10x14_36x52'
  c = _case(name)
  th = 0.3
  inter, area_b = _fused(c, [th], c['fg'], True)
  s_gt, y_gt = _dev(c['s_gt']), _dev(ieo.gt_planes(c['gt_ids'], c['inst_id']))
  conf = torch.ones_like(s_gt)
  areas = inter[:, 0].sum(dim=2).cpu().numpy()
  b, t = np.unravel_index(np.argmax(np.where(areas > 1, -areas, -1e9)), areas.shape)  # the smallest prediction of 2+ pixels
  a = int(areas[b, t])
  assert a > 1
  y_bin = _chain_masks(c, [th], c['fg'], True)[0]
  for tiny, kept in ((a - 1, True), (a, False), (a + 1, False)):
    met = ops.eval_metrics_from_counts(inter, area_b, s_gt, remove_tiny=tiny, conf=conf)[0]
    assert float(met['sizes'][b, t]) == (a if kept else 0) and float(met['conf'][b, t]) == (1.0 if kept else 0.0)
    want_conf = (torch.from_numpy(areas) > tiny).to(torch.float32).cuda()
    assert torch.equal(met['conf'], want_conf)
    y2, conf2 = pp.remove_tiny(y_bin, conf, threshold=tiny)
    ref = ops.eval_metrics(y2.contiguous(), y_gt, s_gt)
    assert torch.equal(met['conf'], conf2)
    for key in ('iou_pairwise', 'stats', 'inst', 'sizes'):
      assert torch.equal(met[key], ref[key]), (tiny, key)
  assert 'conf' not in ops.eval_metrics_from_counts(inter, area_b, s_gt)[0]


def test_output_does_not_depend_on_what_the_memory_held(cuda):
  c = _case('b2_t4_8x12_37x50')
  first = _fused(c, ieo.THRESHOLDS[10], c['fg'], True)
  junk = [torch.full((1 << 16,), 0x7fffffff, dtype=torch.int32, device='cuda') for _ in range(4)]
  del junk  # the caching allocator hands these blocks to the next outputs
  again = _fused(c, ieo.THRESHOLDS[10], c['fg'], True)
  assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])


def test_refusals(cuda):
  c = _case('b1_t3_16x16_16x16')
  yc, ids, inst = _dev(c['yc']), _dev(c['gt_ids']), _dev(c['inst_id'])
  with pytest.raises(rn.RecAttendError, match='>= 0'):
    ops.instance_eval_counts(yc, ids, inst, [0.3, -0.01])
  with pytest.raises(rn.RecAttendError, match='17 thresholds'):
    ops.instance_eval_counts(yc, ids, inst, [0.3] * 17)
  with pytest.raises(rn.RecAttendError, match='T=33'):
    ops.instance_eval_counts(torch.zeros(1, 33, 4, 4, device='cuda'), ids, torch.zeros(1, 33, dtype=torch.int32, device='cuda'), [0.3])
  big = torch.zeros(1, 4097, 4096, dtype=torch.int32, device='cuda')  # one row over 2^24 pixels
  with pytest.raises(rn.RecAttendError, match=r'Hf \* Wf <= 2\^24'):
    ops.instance_eval_counts(yc, big, inst, [0.3])
  del big
  with pytest.raises(rn.RecAttendError, match='CPU tensor'):
    ops.instance_eval_counts(yc.cpu(), ids, inst, [0.3])
  with pytest.raises(rn.RecAttendError, match='CPU tensor'):
    ops.instance_eval_counts(yc, ids, inst, [0.3], fg=torch.zeros(1, 16, 16, dtype=torch.uint8))
  fg = _dev(c['fg']).clone()
  fg[0, 3, 3] = 2
  with pytest.raises(rn.RecAttendError, match='fg holds 2'):
    ops.instance_eval_counts(yc, ids, inst, [0.3], fg=fg)
  with pytest.raises(rn.RecAttendError, match='fg must be uint8'):
    ops.instance_eval_counts(yc, ids, inst, [0.3], fg=fg.to(torch.float32))
  with pytest.raises(rn.RecAttendError, match='int32'):
    ops.instance_eval_counts(yc, ids.to(torch.int64), inst, [0.3])
  # the C entry point itself, on device memory: nothing is launched and the outputs keep what they held
  inter = torch.full((1, 1, 3, 4), 7, dtype=torch.int32, device='cuda')
  area = torch.full((1, 3), 7, dtype=torch.int32, device='cuda')
  neg = np.array([-0.5], np.float32)
  rc = rn.lib().ra_instance_eval_counts_f32(yc.data_ptr(), ids.data_ptr(), inst.data_ptr(), None, 1, 3, 16, 16, 16, 16, 0, neg.ctypes.data,
                                            1, inter.data_ptr(), area.data_ptr(), rn.stream_ptr())
  torch.cuda.synchronize()
  assert rc == rn.RA_E_SHAPE and int(inter.min()) == 7 and int(area.min()) == 7


E2E_SEED = 2


def _e2e_inputs(seed=E2E_SEED):
  rng = np.random.RandomState(seed)
  N, Hf, Wf = 3, 96, 80
  x = rng.rand(N, 64, 64, 3).astype(np.float32)
  rr, cc = np.mgrid[0:Hf, 0:Wf]
  ids = np.zeros((N, Hf, Wf), np.int32)
  for n in range(N):
    for i in range(3):
      cy, cx, rad = rng.uniform(10, Hf - 10), rng.uniform(10, Wf - 10), rng.uniform(8, 20)
      ids[n][(rr - cy) ** 2 + (cc - cx) ** 2 <= rad ** 2] = i + 1
  return x, ids


def _e2e_fg():
  rr, cc = np.mgrid[0:96, 0:80]
  return np.stack([((rr - 48) ** 2 / 40.0 ** 2 + (cc - 40 - 6 * n) ** 2 / 30.0 ** 2 <= 1).astype(np.uint8) for n in range(3)])


def _e2e_model(tmp_path):
  import yaml
  opt = ora.make_opt('cvppp', 64, 64, 2)  # the shapes of smoke()
  res = str(tmp_path / 'results')
  os.makedirs(os.path.join(res, 'm0'))
  with open(os.path.join(res, 'm0', 'model_opt.yaml'), 'w') as f:
    yaml.safe_dump(opt, f)
  np.savez(os.path.join(res, 'm0', 'weights.npz'), **ora.random_params(opt, 1))
  return res, opt


def test_full_model_eval_on_id_images(cuda, tmp_path, monkeypatch):
  """full_model_eval.main on a tiny CVPPP-arch model with an archive of x + gt_instance_ids at 96 x 80 and no y_gt:
  metrics_rank0.yaml holds every default analyzer per threshold, and its means are those of a second run whose archive holds
  the same labels as full-size y_gt planes (the plane path) — on inputs whose band the oracle shows empty, asserted."""
  import yaml
  import full_model
  import full_model_eval
  res, opt = _e2e_model(tmp_path)
  x, ids = _e2e_inputs()
  names = np.array(['a.png', 'b.png', 'c.png'])
  thresholds = [0.3, 0.5]
  # the labels the id path assembles, and the condition on the inputs: an empty band for what this model decodes
  lab = ops.assemble_labels(ids, 64, 64, 2, 'cvppp', want=('inst_id', 's_gt'))
  inst_id, s_gt = lab['inst_id'].cpu().numpy(), lab['s_gt'].cpu().numpy()
  model = full_model.get_model(dict(opt, use_knob=False)).load_weights(dict(np.load(os.path.join(res, 'm0', 'weights.npz'))))
  y_out, s_out = model.run(['y_out', 's_out'], {'x': x, 'phase_train': False}, as_numpy=True)
  yc = (torch.from_numpy(y_out) * torch.from_numpy(s_out)[:, :, None, None]).numpy()  # float32, as apply_confidence forms it
  lo, hi, share, ties = ieo.conditions(ieo.values(yc, 96, 80, False), ids, inst_id, thresholds, None)
  print('end to end: undecided share %.5f, band of %d counts, exact ties %d' % (share, int((hi - lo).sum()), ties))
  assert (lo == hi).all() and ties == 0

  fg = _e2e_fg()
  lo, hi, share, ties = ieo.conditions(ieo.values(yc, 96, 80, True), ids, inst_id, thresholds, fg)
  print('end to end, fg + morph: undecided share %.5f, band of %d counts, exact ties %d' % (share, int((hi - lo).sum()), ties))
  assert (lo == hi).all() and ties == 0

  def run(tag, *flags, **arrays):
    path, out = str(tmp_path / (tag + '.npz')), str(tmp_path / ('out_' + tag))
    np.savez(path, x=x, names=names, **arrays)
    full_model_eval.main(['--model_id', 'm0', '--results', res, '--input', path, '--output', out, '--batch_size', '2',
                          '--threshold_list', '0.3,0.5'] + list(flags))
    with open(os.path.join(out, 'output_valid', 'metrics_rank0.yaml')) as f:
      return yaml.safe_load(f)

  got = run('ids', gt_instance_ids=ids)
  default = ['sbd', 'wt_cov', 'unwt_cov', 'avg_fp', 'avg_fn', 'avg_pr', 'avg_re', 'obj_pr', 'obj_re', 'count_acc', 'count_mse', 'dic',
             'dic_abs']
  assert sorted(got) == ['0.30', '0.50']
  for th in got:
    assert sorted(got[th]) == sorted(default)
  y_gt = ieo.gt_planes(ids, inst_id)
  ref = run('planes', y_gt=y_gt, s_gt=s_gt)
  assert got == ref
  assert any(got[th]['sbd']['mean'] > 0 for th in got) and got['0.30']['sbd']['count'] == 3
  # with a foreground: the mask, the dilation and --remove_tiny on the counted areas against the plane path's
  got_fg = run('ids_fg', '--remove_tiny', '60', gt_instance_ids=ids, fg=fg)
  assert got_fg == run('planes_fg', '--remove_tiny', '60', y_gt=y_gt, s_gt=s_gt, fg=fg.astype(np.float32)) and got_fg != got
  assert got_fg != run('ids_fg_plain', '--remove_tiny', '60', '--no_morph', gt_instance_ids=ids, fg=fg)
  # an archive holding both keys takes the plane path: the counting pass is never called
  monkeypatch.setattr(ops, 'instance_eval_counts', lambda *a, **k: pytest.fail('the id path ran on an archive that holds y_gt'))
  assert run('both', y_gt=y_gt, s_gt=s_gt, gt_instance_ids=ids) == ref
  with pytest.raises(rn.RecAttendError, match='--render cannot be used with an --input that holds gt_instance_ids and no y_gt'):
    full_model_eval.main(['--model_id', 'm0', '--results', res, '--input', str(tmp_path / 'ids.npz'), '--render'])
