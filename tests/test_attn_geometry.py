"""The grid of tests/test_attn_geometry_gpu.py, proved sound on the host before a GPU sees it (tests/attn_geometry_cases.py):
the float64 reference is well conditioned on every record (the same dense operators in float32 stay eight times inside each
tolerance), the kernels' banding rule costs nothing visible, three plausible mistakes in that rule each break the tolerance
on every shape (so the grid can fail), the wholly-outside classes are exact, and the paste cases between them reach every
kernel form the dispatch can return over the grid (ra_paste_plan)."""
import numpy as np
import pytest

import attn_geometry_cases as ag

ALL = tuple(ag.all_shapes())


def _per_record(a):
  return np.abs(a).reshape(a.shape[0], -1).max(axis=1)


def _tols(ref):
  """Per record: (extract, paste, box) tolerances of the GPU tests."""
  n = ref['rec'].shape[0]
  return ag.TOL_EXTRACT * np.maximum(1.0, _per_record(ref['extract'])), np.full(n, ag.TOL_PASTE), np.full(n, ag.TOL_BOX)


def _three(ref, fy, fx, dtype):
  rec = ref['rec'].astype(dtype)
  return (ag.extract_op(ref['img_cv'].astype(dtype), fy, fx), ag.paste_op(ref['P'].astype(dtype), fy, fx, rec), ag.box_op(fy, fx, rec))


def test_grid_is_the_declared_one():
  assert len(ag.CLASS_IDS) == 16 and len(set(ag.CLASS_IDS)) == 16
  for sid in ag.SHAPES:
    rec, pairs = ag.records(sid)
    assert len(pairs) == 48 and len(pairs) % ag.B_LAUNCH == 0
    for axis in (0, 1):  # every class on each axis, three times
      assert sorted(p[axis] for p in pairs) == sorted(ag.CLASS_IDS * 3)
    assert len(set(pairs)) == 48 and (rec[:, 2:4] >= ag.MIN_SIZE).all() and np.isfinite(rec).all()
    # one launch mixes classes
    assert all(len(set(pairs[k:k + ag.B_LAUNCH])) == ag.B_LAUNCH for k in range(0, 48, ag.B_LAUNCH))
  for sid in ag.FORM_ROWS:
    assert {c for p in ag.class_pairs(sid) for c in p} == {'inside', 'edge_lo'}
  H, W, Fh, Fw = ag.SHAPES['s8x320']
  r64 = ag.records('s8x320')[0].astype(np.float64)
  bx = ag.banded_bank(r64[:, 1], r64[:, 3], r64[:, 5], W, Fw)
  cols = [np.flatnonzero(b.any(axis=1)) for b in bx]
  assert max(c[-1] - c[0] + 1 for c in cols if len(c)) > 256   # the extract walks a second column page


@pytest.mark.parametrize('sid', ALL)
def test_float32_reference_is_eight_times_inside_the_tolerances(sid):
  """E32, the float32-against-float64 error of the dense operators, per record and operator: <= tol / 8."""
  ref = ag.reference(sid)
  H, W, Fh, Fw = ag.all_shapes()[sid]
  fy32, fx32 = ag.dense_banks(ref['rec'], H, W, Fh, Fw)
  assert fy32.dtype == np.float32
  worst = {}
  for name, r64, r32, tol in zip(('extract', 'paste', 'box'), (ref['extract'], ref['paste'], ref['box']),
                                 _three(ref, fy32, fx32, np.float32), _tols(ref)):
    assert r32.dtype == np.float32
    ratio = _per_record(r32 - r64) / tol
    k = int(ratio.argmax())
    worst[name] = (round(float(ratio[k]), 4), ref['pairs'][k])
    assert ratio[k] <= 1.0 / ag.CONDITIONING, (name, ref['pairs'][k], ratio[k])
  print(sid, 'E32 / tol:', worst)


@pytest.mark.parametrize('sid', ALL)
def test_banding_is_harmless_and_outside_is_exact(sid):
  ref = ag.reference(sid)
  H, W, Fh, Fw = ag.all_shapes()[sid]
  by, bx = ag.banded_banks(ref['rec'], H, W, Fh, Fw)
  got = _three(ref, by, bx, np.float64)
  for name, r64, rb, tol in zip(('extract', 'paste', 'box'), (ref['extract'], ref['paste'], ref['box']), got, _tols(ref)):
    assert (_per_record(rb - r64) <= tol / ag.CONDITIONING).all(), name
  # a window wholly outside the image: no band holds a pixel, so the extract is exactly 0 and the paste exactly sigmoid(beta)
  o = ref['outside']
  if sid in ag.SHAPES:
    assert o.sum() >= 10
  y_dead = 1.0 / (1.0 + np.exp(-ag.BETA))
  assert (got[0][o] == 0).all() and (got[1][o] == y_dead).all() and (got[2][o] == y_dead).all()


@pytest.mark.parametrize('mutant', ag.MUTANTS)
@pytest.mark.parametrize('sid', tuple(ag.SHAPES))
def test_the_grid_can_fail(sid, mutant):
  """A banded restatement with the band radius halved, half = F / 2 or step = size / F exceeds the tolerance on at least one
  record of every shape of the geometry grid, for the extract and for the paste.  (The form-only rows are there for the
  dispatch: six records of two classes each.)"""
  ref = ag.reference(sid)
  H, W, Fh, Fw = ag.all_shapes()[sid]
  my, mx = ag.banded_banks(ref['rec'], H, W, Fh, Fw, mutant)
  got = _three(ref, my, mx, np.float64)
  tols = _tols(ref)
  for name, r64, rm, tol in (('extract', ref['extract'], got[0], tols[0]), ('paste', ref['paste'], got[1], tols[1])):
    over = _per_record(rm - r64) / tol
    print(sid, mutant, name, 'max error / tol %.3g on %d records' % (over.max(), (over > 1).sum()))
    assert over.max() > 1.5, (name, over.max())   # not by a rounding


def _grid_plans():
  return {(sid, v): ag.paste_plan_str(sid, v) for sid in ag.PASTE_CASES for v in ag.paste_variants(sid)}


def test_paste_cases_name_the_plan_the_dispatch_returns():
  for (sid, v), plan in _grid_plans().items():
    assert plan == ag.PASTE_CASES[sid][v], (sid, v, plan)
  assert set(ag.PASTE_CASES) == set(ag.all_shapes()) - set(ag.EXTRACT_ONLY)


def test_every_paste_form_is_reached_in_both_modes():
  """The general kernel, the window kernel with all rows present and the window kernel with a short last block, each for the
  paste and for the box; and nothing else: a moved threshold fails here or above."""
  plans = _grid_plans()
  for mode in ('paste', 'box'):
    got = {p for (sid, v), p in plans.items() if ag.PASTE_VARIANTS[v]['mode'] == mode}
    assert got == {'general r4 full', 'general r4 short', 'window r4 full', 'window r4 short'}, (mode, got)
  # each condition of the dispatch flips the decode loop's launch at a window shape to the general kernel
  for v in ('chan', 'packed', 'nocanvas', 'stride', 'unaligned', 'box_stride'):
    assert plans[('s40x72', v)].startswith('general') and plans[('s40x72', 'plane')].startswith('window'), v
  for sid in ('s37x50', 's6x1028', 'f_fw80', 'f_fw130', 'f_64x64', 'f_3x3'):   # W % 4, 4 W > 4096, Fw > 64, Fh Fw > 3072, Fh Fw % 4
    assert plans[(sid, 'plane')].startswith('general') and plans[(sid, 'box')].startswith('general'), sid


# shape -> (grid_x, LDS bytes of the general kernel, LDS bytes of the window kernel or None where the shape never reaches it):
# the whole record ra_paste_plan returned before the chooser became a function of its own (rows 4, 256 threads throughout)
PLAN_RECORDS = {'s40x72': (10, 256, 17728), 's37x50': (10, 192, None), 's64x64': (16, 768, 26432), 's6x1028': (2, 256, None),
                's22x40': (6, 192, 17024), 'f_fw80': (10, 1280, None), 'f_fw130': (10, 2080, None), 'f_64x64': (10, 1024, None),
                'f_3x3': (10, 48, None)}
PLAN_FLIPS = {'base': {}, 'no_canvas': dict(has_canvas=False), 'img': dict(has_img=True), 'unaligned': dict(aligned16=False),
              'odd_stride': None}


def test_paste_plan_records_with_each_fact_flipped():
  """ops.paste_plan from the decode loop's facts with each of has_canvas / has_img / aligned16 / the stride flipped on its own,
  paste and box: every field of the record.  A canvas or an image does not count for the box."""
  import ra_ops as ops
  assert set(PLAN_RECORDS) == set(ag.PASTE_CASES)
  for sid, (grid_x, lds_general, lds_window) in PLAN_RECORDS.items():
    H, W, Fh, Fw = ag.all_shapes()[sid]
    for mode in ('paste', 'box'):
      for flip, kw in PLAN_FLIPS.items():
        stride = ag.odd_stride(H, W) if flip == 'odd_stride' else 2 * H * W
        got = ops.paste_plan(mode, ag.B_LAUNCH, H, W, Fh, Fw, y_stride_b=stride, **(kw or {}))
        window = lds_window is not None and (flip == 'base' or (mode == 'box' and flip in ('no_canvas', 'img')))
        want = dict(kernel='window' if window else 'general', rows=4, grid_x=grid_x, threads=256, lds=lds_window if window else lds_general)
        assert got == want, (sid, mode, flip, got)


@pytest.mark.parametrize('sid', tuple(ag.SHAPES))
def test_float32_bank_is_eight_times_inside_its_bound(sid):
  """The dense bank (ra_gaussian_filter_f32's reference) per record and axis: float32 against float64 at an eighth of the GPU
  test's bound of 1e-4 of the bank's largest weight."""
  ref = ag.reference(sid)
  H, W, Fh, Fw = ag.all_shapes()[sid]
  for b32, b64 in zip(ag.dense_banks(ref['rec'], H, W, Fh, Fw), (ref['fy'], ref['fx'])):
    ratio = _per_record(b32 - b64) / np.maximum(1e-6, _per_record(b64)) / 1e-4
    assert ratio.max() <= 1.0 / ag.CONDITIONING, (ref['pairs'][int(ratio.argmax())], ratio.max())


@pytest.mark.parametrize('sid', tuple(ag.ADJOINT_SHAPES))
def test_float32_adjoints_are_eight_times_inside_the_tolerance(sid):
  """The gradients of the dense formulation under torch autograd, float32 against float64, per record and parameter: <= tol / 8
  on every record, the needle class among them (its taps sit on float32-exact positions), so the GPU test keeps it."""
  import torch
  case = ag.adjoint_case(sid)
  n = case['rec'].shape[0]
  assert n == 48 and any('needle' in p for p in case['pairs'])
  (_, g64), (_, g32) = ag.adjoint_reference(case, 0, n, torch.float64), ag.adjoint_reference(case, 0, n, torch.float32)
  excess, at = ag.adjoint_excess(g32, g64)
  k = int(excess.argmax())
  print(sid, 'adjoint E32 / tol: %.4f at %s of %s' % (excess[k], at[k], case['pairs'][k]))
  assert excess[k] <= 1.0 / ag.CONDITIONING, (case['pairs'][k], at[k], excess[k])
  out = np.array([ag.is_outside(p) for p in case['pairs']])
  for name, g in g64.items():   # a window wholly outside the image: the reference's gradients vanish
    assert np.abs(g[out]).max() < 1e-6 * ag.TOL_ADJOINT or name == 'patch', name
