"""Host side of the evaluator's parity table (tests/eval_cases.py): the float32 CPU run of every reference sits CONDITIONING
inside every bar the kernels are held to, the input conditions hold for every row, the rows reach every launch choice they were
chosen for, the restatements the table needs agree with oracle/ra_oracle.py's functions, and one NumPy mutant per family is
rejected by the row built for it, at that row's own bars.  No GPU."""
import numpy as np
import pytest

import eval_cases as ec
import ra_native as rn
import ra_oracle as ora

ALL = [(f, r.name) for f, rows in ec.ROWS.items() for r in rows]
ids = lambda v: '%s-%s' % v if isinstance(v, tuple) else None


@pytest.mark.parametrize('key', ALL, ids=ids)
def test_float32_run_sits_inside_every_bar(key):
  r = ec.ROW_OF[key]
  sc = ec.scores(r, ec.reference(r), ec.reference(r, 'float32'))
  assert sc
  for what, err, bar in sc:
    print('%s %s: %.3g (bar %g)' % (r.name, what, err, bar))
    assert err * ec.CONDITIONING <= bar or (bar == ec.EXACT and err == 0), (what, err, bar)


@pytest.mark.parametrize('key', ALL, ids=ids)
def test_input_conditions(key):
  r = ec.ROW_OF[key]
  cond = ec.conditions(r)
  assert cond, 'no condition checked'
  assert all(cond.values()), [k for k, v in cond.items() if not v]
  x = ec.inputs(r)
  assert all(v.dtype == np.float32 and v.flags['C_CONTIGUOUS'] for v in x.values())
  again, other = ec._INPUTS[r.family](r, False), ec.inputs(r, alt=True)
  assert all(np.array_equal(x[k], again[k]) for k in x)  # seeded
  assert any(not np.array_equal(x[k], other[k]) for k in x)  # the relaunch tests' other draw is another one
  assert max(v.size for v in x.values()) <= 3 * 40000 * 3


@pytest.mark.parametrize('family', list(ec.ROWS))
def test_the_other_draw_meets_the_conditions_too(family):
  """What a relaunch test fills the buffers with first is a valid input of the same row (a few rows per family)."""
  for r in ec.ROWS[family][::max(1, len(ec.ROWS[family]) // 4)]:
    ec._inputs_cached.cache_clear()
    orig = ec._INPUTS[family]
    ec._INPUTS[family] = lambda row, alt, f=orig: f(row, True)
    try:
      cond = ec.conditions(r)
    finally:
      ec._INPUTS[family] = orig
      ec._inputs_cached.cache_clear()
      ec._reference_cached.cache_clear()
    assert all(cond.values()), (r.name, [k for k, v in cond.items() if not v])


def test_the_table_has_the_rows_of_its_dimension_space():
  have = lambda f, **kw: any(all(r.p[k] == v for k, v in kw.items()) for r in ec.ROWS[f])
  for HW in (4, 1020, 1024, 1028):
    for B, T in [(1, 1), (3, 5), (2, 32)] + ([(1, 256)] if HW in (4, 1028) else []):
      for fg in (0, 1):
        for uni in (0, 1):
          for th in (0.5, 0.0, float('-inf')):
            assert have('post', HW=HW, B=B, T=T, fg=fg, uni=uni, thresh=th, shard=1), (HW, B, T, fg, uni, th)
    for T in (1, 5, 32):
      assert have('union', HW=HW, T=T)
      assert all(have('wsum1', HW=HW, T=T, kind=k) for k in ('onehot', 'general', 'zeros'))
  assert have('post', shard=0) and not have('post', HW=1024, T=256)
  for HW in (4, 8188, 8192, 8196, 16388):
    for conf in (0, 1):
      assert all(have('tiny', HW=HW, B=1, T=1, size=s, conf=conf) for s in ('below', 'equal', 'above')) and have('tiny', HW=HW, B=2, T=3, size='all', conf=conf)
  for H, W in [(1, 1), (1, 7), (7, 1), (3, 3), (5, 5), (16, 16), (16, 17), (2, 130)]:
    assert all(have('dilate', H=H, W=W, R=R, vals=v) for R in (0, 2, 16) for v in ('bin', 'real'))
  assert [(r.p['Hs'], r.p['Ws'], r.p['H'], r.p['W']) for r in ec.ROWS['resize']] == [
      (8, 12, 8, 12), (8, 12, 16, 24), (5, 7, 13, 16), (13, 16, 5, 7), (1, 1, 4, 6), (1, 9, 3, 20), (6, 5, 1, 1), (2, 2, 64, 64)]
  for H, W in [(1, 1), (1, 2), (2, 2), (3, 3), (5, 5), (1, 9), (9, 1), (16, 16), (16, 17)]:
    assert all(have('bilateral', kind='plane', H=H, W=W, sc=sc, ss=10.0, vals=v) for sc in (10.0, 0.1) for v in ('smooth', 'bin'))
  assert sum(r.p['kind'] == 'upsample' for r in ec.ROWS['bilateral']) == 2
  for B, T in [(1, 1), (3, 5), (2, 21), (2, 32)]:
    assert have('metrics', kind='tables', B=B, T=T, null='')
  assert all(have('metrics', kind='tables', null=n) for n in ('fg', 'a_in_fgb', 'b_in_fga', 'iou', 'inst'))
  assert [(r.p['B'], r.p['T'], r.p['H'], r.p['W']) for r in ec.ROWS['metrics'] if r.p['kind'] == 'masks'] == [(1, 1, 2, 2), (2, 5, 6, 10), (1, 32, 8, 8)]
  kinds = {k for r in ec.ROWS['metrics'] if r.p['kind'] == 'tables' for k in r.p['kinds']}
  assert kinds == {'full', 'nogt', 'noout', 'part', 'empty'}
  for H, W, C in [(1, 1, 1), (5, 7, 3), (16, 16, 8), (16, 16, 9), (16, 8, 16)]:
    p = ec.TRANSFORM_PAD
    for pad, oy, ox in [(0, 0, 0), (p, 0, 0), (p, p, p), (p, 2 * p, 2 * p - 1), (H + 2, 0, 0)]:
      for fv in (0, 1):
        for fh in (0, 1):
          for tr in ((0, 1) if H == W else (0,)):
            assert have('transform', H=H, W=W, C=C, pad=pad, oy=oy, ox=ox, fv=fv, fh=fh, tr=tr)
  for HW in (1, 255, 16384, 16385, 40000):
    assert all(have('jitter', HW=HW, B=B, draw=d) for B in (1, 3) for d in range(5))
  assert ec.JITTER_DRAWS[0] == (0.0, 1.0, 0.0, 1.0)
  assert ec.inputs(ec.ROW_OF[('jitter', 'hw1-b3-corner1')])['x'].reshape(3, 3).tolist() == [[np.float32(0.4)] * 3, [0, 0, 0], [1, 0, 0]]  # grey, black, red
  assert {tuple(abs(v) for v in d) for d in ec.JITTER_DRAWS[1:]} <= {(0.1, 0.9, 0.1, 0.9), (0.1, 0.9, 0.1, 1.1), (0.1, 1.1, 0.1, 0.9), (0.1, 1.1, 0.1, 1.1)}
  assert len({d for d in ec.JITTER_DRAWS}) == 5 and {d[0] for d in ec.JITTER_DRAWS[1:]} == {0.1, -0.1} == {d[2] for d in ec.JITTER_DRAWS[1:]}
  # the refused calls
  hows = {f: sorted((r.p['how'], r.p['code']) for r in rs) for f, rs in ec.REJECTED.items()}
  for f in ('post', 'union', 'wsum1', 'tiny'):
    assert ('hw15', ec.E_SHAPE) in hows[f] and ('misaligned', ec.E_SHAPE) in hows[f]
  assert ('t257', ec.E_SHAPE) in hows['post'] and ('t33', ec.E_SHAPE) in hows['metrics'] and ('fg-inter-alone', ec.E_INVALID) in hows['metrics']
  assert hows['dilate'] == [('inplace', ec.E_INVALID), ('r17', ec.E_INVALID)]
  assert hows['bilateral'] == [('inplace', ec.E_INVALID), ('sigma-nan', ec.E_INVALID), ('sigma0', ec.E_INVALID)]
  assert hows['transform'] == [('inplace', ec.E_INVALID), ('offset', ec.E_INVALID), ('transpose', ec.E_SHAPE)]
  assert hows['jitter'] == [('short-ws', ec.E_WORKSPACE)]
  assert (rn.RA_E_INVALID, rn.RA_E_SHAPE, rn.RA_E_WORKSPACE) == (ec.E_INVALID, ec.E_SHAPE, ec.E_WORKSPACE)
  assert all((f, r.p['base']) in ec.ROW_OF for f, rs in ec.REJECTED.items() for r in rs)


def test_rows_reach_every_launch_choice():
  """The launch geometry of every row, from the C entry points' own formulas: each choice the table names is taken by a row."""
  ch = {f: [ec.launch_choices(r) for r in rows] for f, rows in ec.ROWS.items()}
  any_ = lambda f, **kw: any(all(c[k] == v for k, v in kw.items()) for c in ch[f])
  # the float4 kernels, grid ceil(HW / 1024): one thread; a workgroup one thread short of full; full; a second with a single thread's float4
  for f in ('post', 'union', 'wsum1'):
    for wg, last in [(1, 1), (1, 255), (1, 256), (2, 1)]:
      assert any_(f, workgroups=wg, last_threads=last), (f, wg, last)
  # s_hard by threadIdx.x < T of block 0: one thread, a few, every thread of the workgroup (the ABI's T = 256), and not at all;
  # T = 256 both where block 0 is the only one with one live pixel thread and where a second block follows
  for T in (1, 5, 32, 256, 0):
    assert any_('post', s_hard_threads=T), T
  assert any_('post', s_hard_threads=256, workgroups=1, last_threads=1) and any_('post', s_hard_threads=256, workgroups=2)
  # remove_tiny, grid ceil(HW / 8192) and a stride of gridDim.x * 1024 pixels: one store; eight passes, the last ragged / full; past 8192: two and
  # three workgroups with a ragged last pass
  for wg, passes, last in [(1, 1, 1), (1, 8, 255), (1, 8, 256), (2, 5, 1), (3, 6, 257)]:
    assert any_('tiny', workgroups=wg, passes=passes, last_pass=last), (wg, passes, last)
  # dilate: windows wider than the image on both axes, one axis, neither; radius 0; a one-pixel-wide plane; two workgroups
  assert any_('dilate', rows_in_window=1, cols_in_window=1) and any_('dilate', rows_in_window=1, cols_in_window=5) and any_('dilate', rows_in_window=5, cols_in_window=1)
  assert any_('dilate', rows_in_window=3, cols_in_window=3, smaller_than_window=True) and any_('dilate', rows_in_window=5, cols_in_window=5, smaller_than_window=False)
  assert any_('dilate', rows_in_window=16, cols_in_window=17, smaller_than_window=True) and any_('dilate', rows_in_window=2, cols_in_window=33, workgroups=2)
  assert any(r.p['R'] == 0 for r in ec.ROWS['dilate']) and any_('dilate', workgroups=2, rows_in_window=16)
  # resize: the copy, an integer ratio, a non-integer one up and down, a 1 x 1 and a 1 x N source, a 1 x 1 result
  for ry, rx in [('same', 'same'), ('up-int', 'up-int'), ('up', 'up'), ('down', 'down'), ('one', 'one'), ('one', 'up')]:
    assert any_('resize', ratio_y=ry, ratio_x=rx), (ry, rx)
  assert any(r.p['H'] * r.p['W'] == 1 and r.p['Hs'] > 1 for r in ec.ROWS['resize']) and any_('resize', workgroups=16)
  # bilateral: reflect101 at n = 1 (always 0), n = 2 (an offset of 2 reflects twice), n = 3 (once), n >= 5; two workgroups
  for lo, hi in [(1, 1), (1, 2), (2, 2), (3, 3), (5, 5), (1, 5)]:
    assert any_('bilateral', n_min=lo, n_max=hi), (lo, hi)
  assert any_('bilateral', workgroups=2)
  twice = ec.reflect_index(np.array([-2, 3]), 2)
  assert twice.tolist() == [0, 1] and ec.reflect_index(np.array([-2, -1, 3, 4]), 3).tolist() == [2, 1, 1, 0]
  # metrics: T*T in one pass of the 256 threads (1, 25 of them), two (441), exactly four (1024)
  for passes, last, live in [(1, 1, 1), (1, 25, 5), (2, 185, 21), (4, 256, 32)]:
    assert any_('metrics', passes=passes, last_pass=last, threads_live=live), (passes, last, live)
  # transform, grid ceil(plane / 2048) and a stride of gridDim.x * 256: one element; a ragged pass; a plane of exactly 2048 (one workgroup, eight
  # full passes), the same in another shape, and past it (two workgroups)
  assert any_('transform', plane=1, workgroups=1, passes=1, last_pass=1) and any_('transform', plane=105, workgroups=1, passes=1, last_pass=105)
  assert any_('transform', plane=2048, workgroups=1, passes=8, last_pass=256) and any_('transform', plane=2304, workgroups=2, passes=5, last_pass=256)
  assert sum(c['plane'] == 2048 for c in ch['transform']) >= 2 * 20
  # jitter, 64 workgroups of 256 always: one pixel (63 idle workgroups), 255 (the same), one pixel per thread exactly, one more, three ragged passes
  for passes, last, idle in [(1, 1, 63), (1, 255, 63), (1, 16384, 0), (2, 1, 0), (3, 40000 - 2 * 16384, 0)]:
    assert any_('jitter', passes=passes, last_pass=last, idle_workgroups=idle), (passes, last, idle)


def test_abi_limits_are_the_ones_the_table_assumes():
  lib = rn.lib()
  assert lib.ra_colour_jitter_workspace_floats(3) == 3 * 64 * 3 and lib.ra_colour_jitter_workspace_floats(0) == 0
  import ra_ops
  assert len(ra_ops.EVAL_NAMES) == 13 and len(ra_ops.EVALI_NAMES) == 6
  assert [ra_ops.EVAL_NAMES[k] for k in ec.EVAL_RATIOS] == ['sbd', 'wt_cov', 'unwt_cov', 'fg_iou', 'fg_dice']
  assert [ra_ops.EVALI_NAMES[k] for k in ec.EVALI_RATIOS] == ['pix_pr', 'pix_re']


# ---- the restatements the table needs are the oracle's functions

def test_post_explicit_is_the_oracle_chain_at_thresholds_from_zero():
  for name in ('hw1028-b3t5-fg-uni-half', 'hw1020-b2t32-nofg-uni-zero', 'hw4-b1t256-fg-half', 'hw1024-b1t1-nofg-half'):
    r = ec.ROW_OF[('post', name)]
    yb, sh = ec.post_explicit(r, ec.inputs(r), np.float64)
    ref = ec.reference(r)
    assert np.array_equal(yb, ref['y_bin']) and np.array_equal(sh, ref['s_hard'])
  r = ec.ROW_OF[('post', 'hw1028-b3t5-nofg-ninf')]  # -inf: utils/postprocess.apply_one_label's call; keep * y is the oracle's apply_one_label
  x = ec.inputs(r)
  y4 = x['y'].astype(np.float64).reshape(3, 5, 1, 1028)
  keep, _ = ec.post_explicit(r, dict(x, s=np.ones_like(x['s'])), np.float64)
  assert np.array_equal(keep.reshape(y4.shape) * y4, ora.pp_apply_one_label(y4))


def test_dilate_restatement_is_pp_morph_at_radius_2():
  for r in ec.ROWS['dilate']:
    if r.p['R'] == 2:
      assert np.array_equal(ec.reference(r)['out'], ora.pp_morph(ec.inputs(r)['y'].astype(np.float64)))


def test_resize_then_bilateral_is_pp_upsample():
  for r in ec.ROWS['bilateral']:
    p, x = r.p, ec.inputs(r)
    y = x['y'] if p['kind'] == 'plane' else ec.resize_ref(x['y'], p['H'], p['W'], np.float64)
    mine = ec.bilateral_ref(y, p['sc'], p['ss'], np.float64)
    assert np.abs(mine - ec.reference(r)['out']).max() < 1e-12, r.name
  for r in ec.ROWS['resize']:  # ... and at sigma_color -> inf, sigma_space -> inf the oracle's filter is a 13-tap box mean of its resize
    p, x = r.p, ec.inputs(r)
    a = ec.resize_ref(x['y'], p['H'], p['W'], np.float64)
    assert np.abs(ec.bilateral_ref(a, 1e9, 1e9, np.float64) - ora.pp_upsample(x['y'], p['H'], p['W'], 1e9, 1e9)).max() < 1e-12, r.name


def test_metrics_restatement_is_eval_metrics_on_masks():
  import ra_ops
  for r in ec.ROWS['metrics']:
    if r.p['kind'] != 'masks':
      continue
    x, ref = ec.inputs(r), ec.reference(r)
    o = ora.eval_metrics(x['y_out'].astype(np.float64), x['y_gt'].astype(np.float64), x['s_gt'].astype(np.float64))
    assert np.abs(o['iou_pairwise'] - ref['iou']).max() < 1e-14
    col = {n: k for k, n in enumerate(ra_ops.EVAL_NAMES)}
    for name, key in [('sbd', 'sbd'), ('wt_cov', 'wt_cov'), ('unwt_cov', 'unwt_cov'), ('fg_iou', 'fg_iou'), ('fg_dice', 'fg_dice'), ('avg_fp', 'avg_fp'),
                      ('avg_fn', 'avg_fn'), ('count_acc', 'count_acc'), ('count_mse', 'count_mse'), ('dic', 'dic'), ('dic_abs', 'dic_abs')]:
      assert np.abs(o[key] - ref['stats'][:, col[name]]).max() < 1e-14, (r.name, name)
    row = {n: k for k, n in enumerate(ra_ops.EVALI_NAMES)}
    inst = ref['inst']
    has_out, is_gt = inst[:, row['has_out']] > 0, inst[:, row['is_gt']] > 0
    for key, name, sel in [('avg_pr', 'pix_pr', has_out), ('obj_pr', 'obj_pr', has_out), ('avg_re', 'pix_re', is_gt), ('obj_re', 'obj_re', is_gt)]:
      mine = inst[:, row[name]][sel]
      assert mine.shape == o[key].shape and np.abs(mine - o[key]).max(initial=0) < 1e-14, (r.name, key)


def test_jitter_restatement_is_colour_jitter():
  for r in ec.ROWS['jitter']:
    d = ec.JITTER_DRAWS[r.p['draw']]
    mine = ec.jitter_ref(ec.inputs(r)['x'], d[0], d[1], d[2], d[3], np.float64)
    assert np.abs(mine - ec.reference(r)['out']).max() < 1e-13, r.name


def test_identity_draws_give_the_image_back():
  for r in ec.ROWS['jitter']:
    if r.p['draw'] == 0:
      assert np.abs(ec.reference(r)['out'] - ec.inputs(r)['x']).max() < 1e-12, r.name


def test_measured_bars_are_what_the_float32_run_gives():
  """A measured bar is CONDITIONING times the float32 CPU run's largest error over its family, one digit up (between that and twice
  it: another NumPy may round an exponential differently); a bar the tree already had is kept where that run sits inside it."""
  m = ec.measure()
  for family, what, bar in [('resize', 'out', ec.TOL_RESIZE), ('jitter', 'out', ec.TOL_JITTER)]:
    e, used, name = m[family][what]
    print(family, what, e, name, bar)
    assert used == bar and ec.CONDITIONING * e <= bar <= 2 * ec.one_digit_up(ec.CONDITIONING * e), (family, e, name)
  for family, what, bar in [('bilateral', 'out', ec.TOL_UPSAMPLE), ('bilateral', 'upsample', ec.TOL_UPSAMPLE), ('wsum1', 'out', ec.TOL_WSUM),
                            ('metrics', 'stats ratios', ec.TOL_METRICS), ('metrics', 'iou_pairwise', ec.TOL_METRICS), ('metrics', 'inst ratios', ec.TOL_METRICS)]:
    e, used, name = m[family][what]
    assert used == bar and ec.CONDITIONING * e <= bar, (family, what, e, name)


# ---- sensitivity: (family, row, mutant, the scores that must fail)
MUTANTS = [
    ('post', 'hw1028-b3t5-fg-uni-half', 'last-max', {'y_bin'}),
    ('post', 'hw4-b1t256-nofg-ninf', 'last-max', {'y_bin'}),
    ('post', 'hw1020-b2t32-nofg-uni-half', 'ge-thresh', {'y_bin', 'union'}),
    ('post', 'hw4-b3t5-nofg-uni-zero', 'ge-thresh', {'y_bin', 'union'}),
    ('union', 'hw1028-t5', 'skip-plane0', {'union'}),
    ('wsum1', 'hw1028-t5-zeros', 'zero-as-one', {'out', 'zero-weight images'}),
    ('wsum1', 'hw4-t32-onehot', 'zero-as-one', {'out'}),
    ('tiny', 'hw16388-6-conf', 'lt', {'y', 'conf'}),
    ('tiny', 'hw4-1-equal-noconf', 'lt', {'y'}),
    ('dilate', '16x17-r2-real', 'zero-border', {'out'}),
    ('dilate', '1x7-r16-real', 'zero-border', {'out'}),
    ('resize', '5x7-13x16', 'align-corners', {'out'}),
    ('resize', '13x16-5x7', 'align-corners', {'out'}),
    ('bilateral', '16x17-sc10-smooth', 'square', {'out'}),
    ('bilateral', '5x5-sc0.1-smooth', 'square', {'out'}),
    ('bilateral', '16x17-sc10-smooth', 'reflect', {'out'}),
    ('bilateral', '3x3-sc10-smooth', 'reflect', {'out'}),
    ('bilateral', 'upsample-5x7-13x16', 'reflect', {'out'}),
    ('metrics', 'b3t5', 'cov-other-axis', {'stats ratios'}),
    ('metrics', 'masks-b2t5-6x10', 'cov-other-axis', {'stats ratios'}),
    ('metrics', 'b2t21', 'sbd-over-T', {'stats ratios'}),
    ('metrics', 'masks-b2t5-6x10', 'sbd-over-T', {'stats ratios'}),
    ('transform', '16x16x8-p3-mid-v1h0t1', 'flips-after-transpose', {'out'}),
    ('transform', '16x16x9-p0-v0h1t1', 'flips-after-transpose', {'out'}),
    ('jitter', 'hw255-b3-corner1', 'one-mean', {'out'}),
    ('jitter', 'hw40000-b1-corner3', 'one-mean', {'out'}),
]


def test_every_family_has_a_mutant():
  assert {m[0] for m in MUTANTS} == set(ec.ROWS) and {(m[0], m[2]) for m in MUTANTS} == {(f, w) for f, ws in ec.MUTANTS.items() for w in ws}


@pytest.mark.parametrize('family,name,which,must_fail', MUTANTS, ids=['%s-%s-%s' % m[:3] for m in MUTANTS])
def test_rows_reject_a_subtly_wrong_kernel(family, name, which, must_fail):
  """The reference passes its own scores; with the error restated on it, the row built for that error fails at its own bars."""
  r = ec.ROW_OF[(family, name)]
  ref = ec.reference(r)
  assert not ec.failures(ec.scores(r, ref, ref))
  failed = set(ec.failures(ec.scores(r, ref, ec.mutant(r, which))))
  print(name, which, sorted(failed))
  assert must_fail <= failed, (must_fail - failed)


def test_mutants_pass_where_the_row_cannot_see_them():
  """The same errors on rows that do not reach them: it is the row that is sharp, not the mutant that is blunt."""
  for family, name, which in [('post', 'hw1028-b1t1-fg-uni-half', 'last-max'), ('post', 'hw1028-b3t5-fg-uni-ninf', 'ge-thresh'), ('union', 'hw1028-t1', 'skip-plane0'),
                              ('wsum1', 'hw1028-t5-general', 'zero-as-one'), ('tiny', 'hw4-1-below-conf', 'lt'), ('dilate', '16x17-r2-bin', 'zero-border'),
                              ('resize', '8x12-8x12', 'align-corners'), ('bilateral', '1x1-sc10-smooth', 'square'), ('bilateral', '1x1-sc10-bin', 'reflect'),
                              ('metrics', 'b1t1', 'sbd-over-T'), ('metrics', 'b1t1', 'cov-other-axis'), ('transform', '16x16x8-p3-mid-v1h1t1', 'flips-after-transpose'),
                              ('transform', '5x7x3-p3-mid-v1h0t0', 'flips-after-transpose'), ('jitter', 'hw255-b3-identity', 'one-mean')]:
    r = ec.ROW_OF[(family, name)]
    ref = ec.reference(r)
    assert not ec.failures(ec.scores(r, ref, ec.mutant(r, which))), (name, which)
