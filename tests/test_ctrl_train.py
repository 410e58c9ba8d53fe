"""Host side of the training controller's parity table (tests/ctrl_train_cases.py): the conditions under which a float32 kernel
can be held to the table's bars, the bounds of the support query, and the saved row's layout.  No GPU."""
import numpy as np
import pytest

import ctrl_train_cases as ct
import ra_native as rn

NAMES = [c.name for c in ct.CASES]


def supported(G=16, Cf=64, hid=32, iters=3, nout=9, n_g=2, n_c=1, mlp=0):
  return rn.lib().ra_ctrl_train_supported_n(G, Cf, hid, iters, nout, n_g, n_c, mlp)


def test_the_table_has_the_rows_it_is_meant_to_have():
  rows = {tuple(c[1:9]) for c in ct.CASES}
  for r in [(16, 64, 256, 5, 2, 1, 0, 3), (56, 64, 256, 5, 2, 1, 0, 2), (256, 64, 256, 5, 2, 1, 0, 2), (ct.G_LDS_BOUND, 64, 256, 5, 2, 1, 0, 1),
            (16, 64, 8, 3, 2, 1, 0, 3), (8, 4, 4, 2, 1, 1, 0, 2), (64, 8, 16, 3, 2, 2, 64, 2), (12, 100, 32, 3, 3, 2, 20, 3),
            (4, 1024, 16, 2, 2, 1, 0, 2), (16, 64, 32, 1, 2, 2, 48, 2), (16, 32, 16, 3, 1, 4, 64, 2), (16, 32, 32, 4, 4, 4, 4, 2)]:
    assert r in rows, r
  for c in ct.CASES:
    assert supported(c.G, c.Cf, c.hid, c.iters, ct.NOUT, c.n_g, c.n_c, c.mlp) == 1, c.name
  # the two rows below hid = 16 are there because the read-out's (1024 / Cf) Cf partial sums outgrow gemv_cols' 16 * 4 hid floats
  for name in ('hid8', 'smallest'):
    c = ct.CASE_OF[name]
    assert (1024 // c.Cf) * c.Cf > 16 * 4 * c.hid
  assert any((1024 // c.Cf) * c.Cf < 1024 and c.Cf > 64 for c in ct.CASES) and any(c.G % 16 for c in ct.CASES)


@pytest.mark.parametrize('name', NAMES)
def test_inputs_are_conditioned(name):
  """No ReLU pre-activation of the float64 run within 1e-4 of its kink, no glimpse map near uniform, and the float32 CPU run of
  the reference CONDITIONING inside every bar the kernels are held to (each scored as the GPU test scores it)."""
  c = ct.CASE_OF[name]
  relu_min, map_peak, (worst, what) = ct.conditions(c)
  print('%s: min |relu pre| %.3g, G max(map) %.3g, float32 run %.3g of the bar at %s' % (name, relu_min, map_peak, worst, what))
  assert relu_min >= ct.RELU_MARGIN
  assert map_peak >= ct.MAP_PEAK
  assert worst * ct.CONDITIONING <= 1.0, what
  if c.iters > 1:  # the conditions are about something: there is a map, and (bar the one-layer MLPs) there are kinks
    assert np.isfinite(map_peak) and (np.isfinite(relu_min) or (c.n_g == 1 and c.n_c == 1))


@pytest.mark.parametrize('name', NAMES)
def test_rows_suffice_for_the_parameter_gradients(name):
  """In float64 the saved rows and pre-activation gradients of the reference give autograd's parameter gradients through
  param_grads_from_rows, for all four combinations: the offsets the GPU test applies to the kernels' rows are the right ones."""
  c = ct.CASE_OF[name]
  ref, x = ct.reference(name), ct.inputs(c)
  for combo in ct.COMBOS:
    g = ref['grads'][combo]
    P = ct.param_grads_from_rows(c, ref['h_last'], ref['save'], ref['save_c'], g, x['dco'] if combo[1] else np.zeros_like(x['dco']))
    for what, err, _ in ct.param_scores(g['params'], P):
      assert err < 1e-12, (combo, what, err)


@pytest.mark.parametrize('name', NAMES)
def test_save_floats_is_the_reference_row_layout(name):
  c = ct.CASE_OF[name]
  n = rn.lib().ra_ctrl_train_save_floats_n(c.G, c.Cf, c.hid, c.iters, c.n_g)
  assert n == c.iters * ct.save_floats(c) == ct.reference(name)['save'][0].size
  f = ct.fields(c)
  assert list(f)[:7] == ['glimpse', 'h_prev', 'gate_i', 'gate_f', 'gate_o', 'gate_u', 'c'] and list(f)[-1] == 'map'
  # the offsets ra_train._CtrlStepBuffers hard-codes: h at Cf, the glimpse MLP's hidden layer l at Cf + 6 hid + l hid
  assert f['h_prev'].start == c.Cf and all(f['z%d' % l].start == c.Cf + 6 * c.hid + l * c.hid for l in range(c.n_g - 1))
  ref = ct.reference(name)['save']
  assert (ref[:, 0, f['h_prev']] == 0).all() and np.allclose(ref[:, 0, f['map']], 1.0 / c.G) and (ref[:, -1, f['c'].stop:f['map'].start] == 0).all()


def test_save_floats_two_layer_entry():
  lib = rn.lib()
  assert lib.ra_ctrl_train_save_floats(16, 64, 256, 5) == lib.ra_ctrl_train_save_floats_n(16, 64, 256, 5, 2) == 5 * (64 + 256 + 6 * 256 + 16)


@pytest.mark.parametrize('what,ok,beyond', [
    ('G % 4', dict(G=16), [dict(G=17), dict(G=18), dict(G=0)]),
    ('Cf % 4', dict(Cf=64), [dict(Cf=66), dict(Cf=65), dict(Cf=0)]),
    ('hid % 4', dict(hid=32), [dict(hid=34), dict(hid=33), dict(hid=0)]),
    ('hid = 4: the smallest', dict(G=8, Cf=4, hid=4), [dict(G=8, Cf=4, hid=2)]),
    ('4 hid <= 1024', dict(hid=256), [dict(hid=260)]),
    ('G <= 4 hid', dict(G=64, Cf=8, hid=16), [dict(G=68, Cf=8, hid=16)]),
    ('Cf <= 1024', dict(G=4, Cf=1024, hid=16), [dict(G=4, Cf=1028, hid=16)]),
    ('mlp <= 4 hid', dict(hid=16, n_c=2, mlp=64), [dict(hid=16, n_c=2, mlp=68)]),
    ('mlp % 4', dict(n_c=2, mlp=4), [dict(n_c=2, mlp=6), dict(n_c=2, mlp=0)]),
    ('mlp unused with one layer', dict(n_c=1, mlp=0), []),
    ('n_g 1..4', dict(n_g=1), [dict(n_g=0)]),
    ('n_g 1..4, top', dict(n_g=4), [dict(n_g=5)]),
    ('n_c 1..4', dict(n_c=1, mlp=32), [dict(n_c=0, mlp=32)]),
    ('n_c 1..4, top', dict(n_c=4, mlp=32), [dict(n_c=5, mlp=32)]),
    ('nout <= 64', dict(nout=64), [dict(nout=65)]),
    ('nout >= 1', dict(nout=1), [dict(nout=0)]),
    ('iters >= 1', dict(iters=1), [dict(iters=0)]),
    ('LDS', dict(G=ct.G_LDS_BOUND, hid=256, iters=5), [dict(G=ct.G_LDS_BOUND + 4, hid=256, iters=5)]),
    ('LDS, two controller layers', dict(G=ct.G_LDS_BOUND, hid=256, n_c=2, mlp=256), [dict(G=ct.G_LDS_BOUND + 4, hid=256, n_c=2, mlp=256)]),
], ids=lambda v: v.replace(' ', '_') if isinstance(v, str) else '')
def test_support_query_bounds(what, ok, beyond):
  """Every bound of ctrl_train_dims_ok: accepted at it, refused one step beyond."""
  assert supported(**ok) == 1, (what, ok)
  for kw in beyond:
    assert supported(**kw) == 0, (what, kw)


def test_lds_boundary_is_the_largest_g_the_query_accepts():
  accepted = [G for G in range(4, 1025, 4) if supported(G=G, hid=256, iters=5)]
  assert max(accepted) == ct.G_LDS_BOUND and accepted == list(range(4, ct.G_LDS_BOUND + 1, 4))
  # the two-layer entry point asks the same question
  assert rn.lib().ra_ctrl_train_supported(ct.G_LDS_BOUND, 64, 256, 5, 9) == 1 and rn.lib().ra_ctrl_train_supported(ct.G_LDS_BOUND + 4, 64, 256, 5, 9) == 0


def test_224_map_stays_refused():
  """224 x 224 gives a 7 x 7 map: G = 49 is no multiple of 4 (the kernels' 16-byte rows), so that size trains on the library path."""
  assert supported(G=49, Cf=64, hid=256, iters=5) == 0
  assert rn.lib().ra_ctrl_train_supported(49, 64, 256, 5, 9) == 0


def test_scores_catch_wrong_results():
  """The float32 CPU run passes every score; with two gates swapped in the saved rows, one image's d feat zeroed, the glimpse
  MLP's first-layer gradient rows not shifted against their inputs, or d feat off by 1e-4 of itself, the scores fail."""
  name = 'cf100'
  c, ref, r32 = ct.CASE_OF[name], ct.reference(name), ct.reference(name, 'float32')
  f, combo = ct.fields(c), ct.COMBOS[0]
  fails = lambda scores: [w for w, e, bar in scores if not e < bar]
  assert not fails(ct.all_scores(c, ref, r32))
  save = r32['save'].copy()
  save[:, :, f['gate_f']], save[:, :, f['gate_o']] = r32['save'][:, :, f['gate_o']], r32['save'][:, :, f['gate_f']]
  assert fails(ct.forward_scores(c, ref, dict(r32, save=save))) == ['save.gate_f', 'save.gate_o']
  g = {k: np.array(v) if k != 'params' else v for k, v in r32['grads'][combo].items()}
  assert np.abs(g['dfeat']).max() < 1.0  # a floor of 1 on the scale would let the next two pass
  for wrong in (np.concatenate([g['dfeat'][:1] * 0, g['dfeat'][1:]]), g['dfeat'] * (1 + 1e-4)):
    assert fails(ct.grad_scores(c, ref['grads'][combo], dict(g, dfeat=wrong), combo)) == ['dfeat']
  rolled = dict(g, dzg=np.roll(g['dzg'], 1, axis=2))
  P = ct.param_grads_from_rows(c, r32['h_last'], r32['save'], r32['save_c'], rolled, ct.inputs(c)['dco'])
  assert {'d glimpse_mlp_w_0', 'd glimpse_mlp_w_1'} <= set(fails(ct.param_scores(ref['grads'][combo]['params'], P)))
