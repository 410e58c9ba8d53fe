"""Float64 parity of the training controller's two kernels (csrc/ra_ctrl_train.hip) over their dimension space, through the C ABI.

The rows, the reference and the bars are in tests/ctrl_train_cases.py; tests/test_ctrl_train.py asserts on the host that the
float32 CPU run of the reference sits 8 times inside every bar used here.  Every output lies in a buffer of sentinel words and
starts as NaN, so a hole or a write outside is seen whatever a previous launch left in memory.  Per row:
  forward   h_last, co and every field of the saved rows against float64; the last iteration's saved z exactly zero; a launch
            into buffers another input has filled gives the bits of a launch into fresh ones.
  backward  with d h_last and d co each present or absent: d feat and every pre-activation gradient per image on that image's
            own |ref| maximum; what is identically zero exactly zero; dzc untouched where d co is absent; the parameter gradients
            formed from the kernels' OWN rows at ra_train._CtrlStepBuffers' offsets against autograd's.
A row that fails its float64 forward comparison with `red` carved as 16 * 4 hid again: hid8 (see test_forward's docstring)."""
import numpy as np
import pytest
import torch

import ctrl_train_cases as ct

pytestmark = pytest.mark.gpu

NAMES = [c.name for c in ct.CASES]


def _assert_scores(scores, what):
  bad = []
  for w, e, bar in scores:
    print('%s %s: %.3g (bar %g)' % (what, w, e, bar))
    if not e < bar:
      bad.append((w, e, bar))
  assert not bad, '%s: %s' % (what, bad)


def _bits(r):
  return b''.join(np.ascontiguousarray(r[k]).tobytes() for k in ('h_last', 'co', 'save', 'save_c'))


@pytest.mark.parametrize('name', NAMES)
def test_forward(cuda, name):
  """Values against float64 and the exact properties.

  What the hid8 row (G 16, Cf 64, hid 8) sees of a scratch of 16 * 4 hid = 512 floats: the read-out writes red[0, 1024), so its
  parts 8..15 land on xh [72], cst [8], va [32], gm [16] and the first 384 floats of the feature map.  The first iteration then
  starts from partial sums (feat[9, c] / 16, half of them non-zero) as h and c instead of zeros, and positions 0..5 of the map
  hold partial sums for every read-out that follows: the saved h_prev of iteration 0, which must be exactly zero, is not, and
  the gates and all behind them leave their float64 values at the 1e-2 level, against bars of 5e-5.  At the smallest row
  (G 8, Cf 4, hid 4) the 1024 partial sums run past the 324 floats of LDS the launch asked for altogether."""
  c = ct.CASE_OF[name]
  xd = ct.device_inputs(c, cuda)
  first = ct.forward_buffers(c, cuda)
  ct.launch_forward(c, xd, xd['feat'], first)
  got = ct.forward_results(c, first, name + ' forward')
  _assert_scores(ct.forward_scores(c, ct.reference(name), got), name)
  f = ct.fields(c)
  assert (got['save'][:, -1, f['c'].stop:f['map'].start] == 0).all(), 'the last iteration\'s saved z is not exactly zero'
  assert (got['save'][:, 0, f['h_prev']] == 0).all() and (got['save'][:, 0, f['map']] == np.float32(1.0) / np.float32(c.G)).all()
  # the same buffers after another input, then this one again: nothing of the other launch is left, and the bits repeat
  again = ct.forward_buffers(c, cuda)
  ct.launch_forward(c, xd, xd['feat2'], again)
  other = ct.forward_results(c, again, name + ' forward, other features')
  assert not np.array_equal(other['save'], got['save']) and not np.array_equal(other['co'], got['co'])
  ct.launch_forward(c, xd, xd['feat'], again)
  assert _bits(ct.forward_results(c, again, name + ' forward, relaunched')) == _bits(got)


@pytest.mark.parametrize('name', NAMES)
def test_backward(cuda, name):
  c = ct.CASE_OF[name]
  ref, x = ct.reference(name), ct.inputs(c)
  xd = ct.device_inputs(c, cuda)
  fwd = ct.forward_buffers(c, cuda)
  ct.launch_forward(c, xd, xd['feat'], fwd)
  saved = ct.forward_results(c, fwd, name + ' forward')
  for combo in ct.COMBOS:
    what = '%s %s' % (name, ct.combo_id(combo))
    g, rg = ct.launch_backward(c, xd, fwd, combo, cuda), ref['grads'][combo]
    _assert_scores(ct.grad_scores(c, rg, g, combo), what)
    # identically zero in the reference: exactly zero here
    assert (g['dlog'][:, -1] == 0).all() and (g['dzg'][:, :, -1] == 0).all(), what
    if combo == (False, False):
      assert all((g[k] == 0).all() for k in ('dfeat', 'dpre', 'dlog', 'dzg')), what
    if not combo[1]:  # begin_step zeroes the dzc rows once and relies on a backward without d co leaving them alone
      assert (g['dzc'] == np.float32(ct.DZC_FILL)).all(), what + ': dzc written without d co'
      g = dict(g, dzc=np.zeros_like(rg['dzc']))
    P = ct.param_grads_from_rows(c, saved['h_last'], saved['save'], saved['save_c'], g, x['dco'] if combo[1] else np.zeros_like(x['dco']))
    _assert_scores(ct.param_scores(rg['params'], P), what)
  again = ct.launch_backward(c, xd, fwd, ct.COMBOS[0], cuda)  # two launches: the same bits
  first = ct.launch_backward(c, xd, fwd, ct.COMBOS[0], cuda)
  assert all(first[k].tobytes() == again[k].tobytes() for k in first)


@pytest.mark.parametrize('name', ['depth4', 'cf100'])
def test_backward_layer_strides(cuda, name):
  """dzg / dzc with their layers further apart than one layer, as the stacked step's 'all' view of [layers][T, B, ...] has
  them: the same bits as the dense launch, and the floats between the layers untouched (launch_backward checks them)."""
  c = ct.CASE_OF[name]
  assert c.n_g > 2 and c.n_c > 1
  xd = ct.device_inputs(c, cuda)
  fwd = ct.forward_buffers(c, cuda)
  ct.launch_forward(c, xd, xd['feat'], fwd)
  for combo in ct.COMBOS[:3]:
    dense, strided = ct.launch_backward(c, xd, fwd, combo, cuda), ct.launch_backward(c, xd, fwd, combo, cuda, gap=36)
    for k in dense:
      assert dense[k].tobytes() == strided[k].tobytes(), (ct.combo_id(combo), k)
    if combo[0] and combo[1]:
      _assert_scores(ct.grad_scores(c, ct.reference(name)['grads'][combo], strided, combo), name + ' strided')
