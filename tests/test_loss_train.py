"""Host side of the loss-side parity table (tests/loss_train_cases.py): the float32 CPU run of every reference sits CONDITIONING
inside every bar the kernels are held to, the input conditions hold for every row, the rows reach every launch choice they were
chosen for, and one NumPy mutant per plausible kernel error is rejected by the row built for it, at that row's own bars.  No GPU."""
import numpy as np
import pytest
import torch

import loss_train_cases as lt
import ra_native as rn

ALL = [(f, r.name) for f, rows in lt.ROWS.items() for r in rows]
ids = lambda v: '%s-%s' % v if isinstance(v, tuple) else None


@pytest.mark.parametrize('key', ALL, ids=ids)
def test_float32_run_sits_inside_every_bar(key):
  r = lt.ROW_OF[key]
  for what, err, bar in lt.scores(r, lt.reference(r), lt.reference(r, 'float32')):
    print('%s %s: %.3g (bar %g)' % (r.name, what, err, bar))
    assert err * lt.CONDITIONING <= bar or (bar == lt.EXACT and err == 0), (what, err, bar)


@pytest.mark.parametrize('key', ALL, ids=ids)
def test_input_conditions(key):
  r = lt.ROW_OF[key]
  cond = lt.conditions(r)
  assert cond or r.family == 'canvas', 'no condition checked'
  assert all(cond.values()), [k for k, v in cond.items() if not v]
  x = lt.inputs(r)
  assert all(v.dtype == np.float32 and v.flags['C_CONTIGUOUS'] for v in x.values())
  again, other = lt.inputs(r), lt.inputs(r, alt=True)
  assert all(np.array_equal(x[k], again[k]) for k in x)  # seeded
  assert any(not np.array_equal(x[k], other[k]) for k in x)  # the relaunch tests' other draw is another one


def test_the_table_has_the_rows_the_bars_were_chosen_at():
  have = lambda f, **kw: any(all(r.p[k] == v for k, v in kw.items()) for r in lt.ROWS[f])
  for B, T in [(1, 1), (3, 5), (4, 8), (5, 9), (2, 32), (2, 64), (256, 2)]:
    assert have('head', B=B, T=T, ties=False), (B, T)
  assert have('head', B=3, T=5, ties=True) and have('head', B=5, T=9, ties=True)
  assert {r.p['mix'] for r in lt.ROWS['head']} == {0.0, 1.0, 0.3} and {r.p['HW'] for r in lt.ROWS['head']} == {16, 262144}
  assert {r.p['g'] for r in lt.ROWS['head']} >= {None} and any(r.p['g'] not in (None, 1.0) for r in lt.ROWS['head'])
  assert all(r.p['mix'] != 0 for r in lt.ROWS['head'] if r.p['ties'])
  assert [(r.p['B'], r.p['T']) for r in lt.HEAD_REJECTED] == [(257, 2), (2, 65)]
  for B, T in [(1, 1), (3, 5), (2, 21), (5, 32)]:
    for fixed in (0, 1):
      for fn in (0, 1):
        assert have('stats', B=B, T=T, fixed=fixed, fn=fn)
  for HW in (4, 1020, 1024, 1028):
    for N, T in [(1, 1), (3, 5), (32, 32)]:
      assert have('wsum', HW=HW, N=N, T=T, bias=0, B=3) and have('wsum', HW=HW, N=N, T=T, bias=1, B=3)
  for HW in (255, 256, 257):
    for C, cc in [(4, 3), (4, 0), (8, 5), (12, 11)]:
      for form in lt.CANVAS_FORMS:
        assert have('canvas', HW=HW, C=C, cc=cc, form=form, B=3)
  assert {r.p['knob_stride'] for r in lt.ROWS['canvas'] if r.p['form'] != 'nomatch'} == {1, 3}
  for N, M in [(1, 1), (16, 16), (17, 16), (16, 17), (17, 17), (32, 32)]:
    assert have('pair', N=N, M=M, HW=64)
  assert all(have('pair', N=17, M=17, HW=HW) for HW in (4, 4092, 4096, 4100)) and have('pair', N=2, M=2, HW=9 * 4096)
  for H, W in [(4, 4), (6, 4), (40, 36)]:
    for B, T in lt.BOX_BT:
      assert have('box', H=H, W=W, B=B, T=T)
  assert lt.BOX_BT == [(1, 1), (8, 8), (5, 13), (2, 9), (2, 16), (2, 17), (1, 32)]
  assert have('box', H=64, W=64) and have('box', H=64, W=68) and have('box', H=516, W=512)


def test_rows_reach_every_launch_choice():
  """The launch geometry of every row, from the C entry points' own formulas: each choice the table names is taken by a row."""
  ch = {f: [lt.launch_choices(r) for r in rows] for f, rows in lt.ROWS.items()}
  any_ = lambda f, **kw: any(all(c[k] == v for k, v in kw.items()) for c in ch[f])
  # loss head: an idle wave, one image per wave, a wave's second image, the 64th; T*T below, at and past one pass of the lanes
  assert any_('head', idle_waves=3) and any_('head', idle_waves=1) and any_('head', images_per_wave=1, idle_waves=0)
  assert any_('head', images_per_wave=2) and any_('head', images_per_wave=64, last_slot=255)
  assert any_('head', passes=1, last_pass=1) and any_('head', passes=1, last_pass=64) and any_('head', passes=2, last_pass=17)
  assert any_('head', passes=64, last_pass=64, lanes_live=64) and any_('head', lanes_live=32)
  # statistics: one row, an odd count, 32
  assert {c['rows_live'] for c in ch['stats']} == {1, 5, 21, 32}
  # weighted sum: one thread; a last workgroup one thread short of full; full; a second one with one live thread
  for wg, last in [(1, 1), (1, 255), (1, 256), (2, 1)]:
    assert any_('wsum', workgroups=wg, last_threads=last), (wg, last)
  # canvas: 255 / 256 threads of one workgroup, a second with one; every (group, lane) of the table, in 1, 2 and 3 groups
  for wg, last in [(1, 255), (1, 256), (2, 1)]:
    assert any_('canvas', workgroups=wg, last_threads=last), (wg, last)
  for groups, group, lane in [(1, 0, 3), (1, 0, 0), (2, 1, 1), (3, 2, 3)]:
    assert any_('canvas', groups=groups, group=group, lane=lane)
  # pair statistics: the four templates; one short chunk, one a group short, one full, a second of four pixels; nine chunks
  for NI, NJ in [(1, 1), (1, 2), (2, 1), (2, 2)]:
    assert any_('pair', NI=NI, NJ=NJ), (NI, NJ)
  for chunks, last in [(1, 4), (1, 4092), (1, 4096), (2, 4)]:
    assert any_('pair', chunks=chunks, last_chunk_px=last, NI=2, NJ=2), (chunks, last)
  assert any_('pair', chunks=9, chunks_mod8=1)
  # boxes: empty slices, a short slice, eight full ones; TM at and past its boundaries; B T = 64 and 65; nblk 1, 2 and capped
  assert any_('box', slices_empty=4) and any_('box', slices_empty=2) and any_('box', slices_empty=0, slices_short=0) and any_('box', slices_short=1)
  Ts = lambda TM: {r.p['T'] for r in lt.ROWS['box'] if lt.launch_choices(r)['TM'] == TM}
  assert Ts(8) >= {1, 8} and Ts(16) >= {9, 13, 16} and Ts(32) >= {17, 32}
  assert any_('box', workgroups=1, last_threads=64) and any_('box', workgroups=2, last_threads=1) and any_('box', workgroups=1, last_threads=1)
  assert any_('box', nblk=1, passes=4, cap_binds=False) and any_('box', nblk=2, cap_binds=False) and any_('box', nblk=64, cap_binds=True, passes=5)
  # below the cap a thread takes at most four 16-byte loads; 516 x 512 is the smallest map (W a multiple of 4, H >= W) at which
  # the cap binds, and a fifth pass follows
  assert all(c['passes'] <= 4 for c in ch['box'] if not c['cap_binds'])
  assert -(-(512 * 512 // 4) // 1024) == 64 and -(-(516 * 512 // 4) // 1024) == 65


def test_abi_limits_are_the_ones_the_table_assumes():
  lib = rn.lib()
  assert lib.ra_loss_stats_workspace_floats(5) == 60 and lib.ra_gt_box_workspace_floats(2, 3) == 2 * 3 * 8 * 5
  assert lib.ra_box_iou_rects_workspace_floats(2) == 2 * 64 * 33
  assert lib.ra_pair_stats_workspace_floats(3, 4100) == 3 * (2 + 1) * (2 * 32 * 32 + 3 * 32)


@pytest.mark.parametrize('name', [r.name for r in lt.ROWS['head'] if not r.p['ties']])
def test_index_rule_is_autograd_where_no_scores_tie(name):
  """d s_out by the explicit index rule equals torch autograd's through cummin / cummax in float64 wherever the scores differ."""
  r = lt.ROW_OF[('head', name)]
  ref = lt.reference(r)
  rule = lt.head_ds(lt.inputs(r), r.p, np.float64)
  assert np.abs(rule - ref['ds_autograd']).max() <= 1e-12 * max(1.0, np.abs(rule).max())


@pytest.mark.parametrize('name', [r.name for r in lt.ROWS['head'] if r.p['ties']])
def test_cpu_cummin_takes_the_documented_positions(name):
  """What recattend.h documents: on the CPU torch.cummin reports the last position of the running minimum, flip(cummax(flip))
  the smallest index >= t holding the maximum of s[t..T) — the rule cum_ext_indices states, on the planted ties."""
  r = lt.ROW_OF[('head', name)]
  s = lt.inputs(r)['s_out']
  for b in range(r.p['B']):
    imin, imax = lt.cum_ext_indices(s[b])
    t = torch.from_numpy(s[b]).to(torch.float64)
    T = len(s[b])
    assert torch.cummin(t, 0)[1].tolist() == imin.tolist()
    assert (T - 1 - torch.flip(torch.cummax(torch.flip(t, [0]), 0)[1], [0])).tolist() == imax.tolist()
  ref = lt.reference(r)
  assert np.abs(ref['ds'] - ref['ds_autograd']).max() <= 1e-9 * np.abs(ref['ds']).max()  # so autograd on the CPU agrees here too
  assert np.array_equal(ref['pieces'], lt.mutant(r, 'other-tie')['pieces'])            # the loss does not depend on the rule


def test_the_two_oracles_state_one_pairwise_iou():
  for r in lt.ROWS['pair'][:5]:
    ref = lt.reference(r)
    assert np.abs(ref['iou_soft'] - ref['iou_soft_torch']).max() < 1e-14


# ---- sensitivity: (family, row, mutant, the scores that must fail)
MUTANTS = [
    ('pair', 'n17m17-hw4096', 'chunk-tail', {'sum_a', 'sum_b', 'inter', 'iou_soft', 'sum_a_hard'}),
    ('pair', 'n2m2-hw36864', 'chunk-tail', {'sum_a', 'sum_a_hard'}),
    ('head', 'b5t9', 'stale-coef', {'ds'}),
    ('head', 'b5t9-ties', 'stale-coef', {'ds'}),
    ('head', 'b3t5', 'no-clamp', {'pieces'}),
    ('head', 'b3t5-ties', 'other-tie', {'ds'}),
    ('head', 'b5t9-ties', 'other-tie', {'ds'}),
    ('box', '40x36-b8t8', 'tm-1', {'iou'}),
    ('box', '40x36-b2t16', 'tm-1', {'iou'}),
    ('box', '40x36-b1t32', 'tm-1', {'iou'}),
    ('box', '40x36-b2t9', 'last-slice', {'params'}),
    ('box', '40x36-b8t8', 'last-slice', {'params'}),
    ('canvas', 'hw257-c8cc5-noise', 'group0', {'canvas channel', 'copied channels'}),
    ('canvas', 'hw255-c12cc11-nomatch', 'group0', {'canvas channel', 'copied channels'}),
    ('wsum', 'hw1028-n3t5-bias', 'zero-row', {'zero-weight rows'}),
    ('wsum', 'hw4-n1t1-bias', 'zero-row', {'zero-weight rows'}),
]


@pytest.mark.parametrize('family,name,which,must_fail', MUTANTS, ids=['%s-%s-%s' % m[:3] for m in MUTANTS])
def test_rows_reject_a_subtly_wrong_kernel(family, name, which, must_fail):
  """The reference passes its own scores; with the error restated on it, the row built for that error fails at its own bars."""
  r = lt.ROW_OF[(family, name)]
  ref = lt.reference(r)
  assert not lt.failures(lt.scores(r, ref, ref))
  failed = set(lt.failures(lt.scores(r, ref, lt.mutant(r, which))))
  print(name, which, sorted(failed))
  assert must_fail <= failed, (must_fail - failed)


def test_mutants_pass_where_the_row_cannot_see_them():
  """The same errors on rows that do not reach them: it is the row that is sharp, not the mutant that is blunt."""
  for family, name, which in [('pair', 'n17m17-hw4092', 'chunk-tail'), ('head', 'b4t8', 'stale-coef'), ('head', 'b5t9', 'other-tie'),
                              ('box', '40x36-b2t9', 'tm-1'), ('canvas', 'hw256-c4cc3-noise', 'group0'), ('wsum', 'hw1024-n3t5-nobias', 'zero-row')]:
    r = lt.ROW_OF[(family, name)]
    ref = lt.reference(r)
    assert not lt.failures(lt.scores(r, ref, lt.mutant(r, which))), (name, which)


@pytest.mark.parametrize('name', lt.names('box'))
def test_knob_chain_is_the_oracle_in_float32(name):
  """The element-wise float32 chain ra_knob_setup_f32 is held to bit for bit is oracle/ra_oracle.py's get_gt_box run in float32."""
  r = lt.ROW_OF[('box', name)]
  ref, r32 = lt.reference(r), lt.reference(r, 'float32')
  assert np.array_equal(ref['ctr_chain'].astype(np.float64), r32['ctr']) and np.array_equal(ref['size_chain'].astype(np.float64), r32['size'])
