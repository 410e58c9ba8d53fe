"""Float64 parity of the loss side of the training step over its dimension space, through the C ABI: ra_loss_head_f32 and its
backward, ra_loss_stats_f32, ra_weighted_sum_multi_f32 (dense and strided), ra_canvas_step_f32, ra_pair_stats_f32 (dense and
strided) and ra_gt_box_f32 -> ra_knob_setup_f32 -> ra_box_iou_rects_f32.

The rows, the references and the bars are in tests/loss_train_cases.py; tests/test_loss_train.py asserts on the host that the
float32 CPU run of every reference sits 8 times inside every bar used here and that the rows reach the launch choices they were
chosen for.  Every output lies in a buffer of sentinel words and starts as NaN, so a hole or a write outside is seen whatever a
previous launch left in memory.  Per family: every row against float64, a launch into buffers another input has filled giving
the bits of a launch into fresh ones (every sum here has a fixed order), and the refused shapes with their outputs untouched."""
import numpy as np
import pytest
import torch

import loss_train_cases as lt

pytestmark = pytest.mark.gpu


def _assert_scores(scores, what):
  bad = []
  for w, e, bar in scores:
    print('%s %s: %.3g (bar %g)' % (what, w, e, bar))
    if not e < bar:
      bad.append((w, e, bar))
  assert not bad, '%s: %s' % (what, bad)


def _row(family, name):
  return lt.ROW_OF[(family, name)]


def _parity(r, cuda, form=None):
  bufs, got = lt.launch(r, lt.inputs(r), cuda, form=form)
  _assert_scores(lt.scores(r, lt.reference(r), got), '%s %s%s' % (r.family, r.name, ' ' + form if form else ''))
  return bufs, got


def _bytes(got):
  return b''.join(np.ascontiguousarray(got[k]).tobytes() for k in sorted(got))


def _relaunch(r, cuda, fresh, form=None):
  """Another draw of the inputs into new buffers, then the row's own into the same ones: the bits of the launch into fresh ones."""
  bufs, other = lt.launch(r, lt.inputs(r, alt=True), cuda, form=form)
  assert _bytes(other) != _bytes(fresh), 'the other draw gave the same results: the relaunch shows nothing'
  _, again = lt.launch(r, lt.inputs(r), cuda, bufs=bufs, form=form)
  for k in fresh:
    assert np.ascontiguousarray(again[k]).tobytes() == np.ascontiguousarray(fresh[k]).tobytes(), (r.name, k)


def _assert_refused(call, bufs, code, what):
  """call() returns its code(s) without a launch: the guarded buffers keep every bit."""
  import ra_native as rn
  guarded = lt.guarded_only(bufs)
  before = lt.bits_of(guarded)
  rcs = call()
  for rc in (rcs if isinstance(rcs, tuple) else (rcs,)):
    assert rc == code, '%s: returned %d, not %d (%s)' % (what, rc, code, (rn.lib().ra_last_error_string() or b'').decode())
  assert lt.bits_of(guarded) == before, '%s: a refused call wrote to its outputs' % what


# ---- the loss head

@pytest.mark.parametrize('name', lt.names('head'))
def test_loss_head(cuda, name):
  """pieces (six floats: the guard behind them is what settles recattend.h's [0..5] against the eight ra_train.LossHead
  allocates), c1 / c0 of both adjoints, d s_out; the tie rows against the explicit index rule."""
  _parity(_row('head', name), cuda)


@pytest.mark.parametrize('name', ['b5t9', 'b5t9-ties', 'b2t64'])
def test_loss_head_relaunch(cuda, name):
  r = _row('head', name)
  _relaunch(r, cuda, lt.launch(r, lt.inputs(r), cuda)[1])


@pytest.mark.parametrize('r', lt.HEAD_REJECTED, ids=[r.name for r in lt.HEAD_REJECTED])
def test_loss_head_refuses_beyond_its_limits(cuda, r):
  bufs = lt.head_buffers(r, cuda)
  xd = lt.to_dev(lt.inputs(r), cuda)
  _assert_refused(lambda: lt.head_call(r, xd, bufs), bufs, lt.E_SHAPE, r.name)


# ---- the statistics

@pytest.mark.parametrize('name', lt.names('stats'))
def test_loss_stats(cuda, name):
  """All 15 statistics; the counts (count_acc, dic, dic_abs) as the float32 of the exact ratio."""
  _parity(_row('stats', name), cuda)


@pytest.mark.parametrize('name', ['b5t32-match-iou', 'b3t5-fixed-wtcov'])
def test_loss_stats_relaunch(cuda, name):
  r = _row('stats', name)
  _relaunch(r, cuda, lt.launch(r, lt.inputs(r), cuda)[1])


def test_loss_stats_refuses_t33(cuda):
  r = _row('stats', 'b5t32-match-iou')
  bufs = lt.stats_buffers(r, cuda)
  xd = lt.to_dev(lt.inputs(r), cuda)
  _assert_refused(lambda: lt.stats_call(r, xd, bufs, T=33), bufs, lt.E_SHAPE, 'T = 33')


# ---- the weighted sum

@pytest.mark.parametrize('name', lt.names('wsum'))
def test_weighted_sum_multi(cuda, name):
  """Dense, timestep-major through strides, and timestep-major with rows further apart (the floats between keep their
  sentinel): each against float64, a row of zero weights equal to the bias bit for bit, the three forms the same bits."""
  r = _row('wsum', name)
  got = {form: _parity(r, cuda, form)[1]['out'] for form in lt.WSUM_FORMS}
  for form in lt.WSUM_FORMS[1:]:
    assert got[form].tobytes() == got['dense'].tobytes(), form


@pytest.mark.parametrize('name,form', [('hw1028-n3t5-bias', 'dense'), ('hw1028-n32t32-nobias', 'tmajor'), ('hw1020-n3t5-bias', 'tmajor-gap')])
def test_weighted_sum_multi_relaunch(cuda, name, form):
  r = _row('wsum', name)
  _relaunch(r, cuda, lt.launch(r, lt.inputs(r), cuda, form=form)[1], form=form)


def test_weighted_sum_multi_refuses_misaligned_strides(cuda):
  r = _row('wsum', 'hw1028-n3t5-bias')
  HW, B = r.p['HW'], r.p['B']
  xd = lt.to_dev(lt.inputs(r), cuda)
  bufs = lt.wsum_buffers(r, cuda, 'tmajor-gap')
  for strides in [(HW + 2, B * HW + 8), (HW, B * HW + 6), (HW + 1, B * HW + 8)]:
    _assert_refused(lambda: lt.wsum_call(r, xd, bufs, 'tmajor-gap', strides=strides), bufs, lt.E_SHAPE, 'strides %r' % (strides,))


# ---- the canvas step

@pytest.mark.parametrize('name', lt.names('canvas'))
def test_canvas_step(cuda, name):
  """The canvas channel bit for bit against the element-wise float32 chain; every other channel a bit copy of inp_prev."""
  _parity(_row('canvas', name), cuda)


@pytest.mark.parametrize('name', ['hw257-c8cc5-noise', 'hw255-c12cc11-nomatch'])
def test_canvas_step_relaunch(cuda, name):
  r = _row('canvas', name)
  _relaunch(r, cuda, lt.launch(r, lt.inputs(r), cuda)[1])


def test_canvas_step_refuses_bad_channels(cuda):
  import ra_native as rn
  r = _row('canvas', 'hw257-c8cc5-noise')
  xd = lt.to_dev(lt.inputs(r), cuda)
  bufs = lt.canvas_buffers(r, cuda)
  for C, cc in [(6, 5), (8, 8), (8, -1)]:
    bad = r._replace(p=dict(r.p, C=C, cc=cc))
    _assert_refused(lambda: lt.canvas_call(bad, xd, bufs), bufs, rn.RA_E_INVALID, 'C %d cc %d' % (C, cc))


# ---- the pairwise statistics

@pytest.mark.parametrize('name', lt.names('pair'))
def test_pair_stats(cuda, name):
  """All seven outputs, inter and sum_a_hard included; a dense and a timestep-major in place: the same bits."""
  r = _row('pair', name)
  dense, tmajor = _parity(r, cuda)[1], _parity(r, cuda, 'tmajor')[1]
  for k in dense:
    assert dense[k].tobytes() == tmajor[k].tobytes(), k


@pytest.mark.parametrize('name,form', [('n17m17-hw4100', None), ('n2m2-hw36864', 'tmajor'), ('n16m17-hw64', None)])
def test_pair_stats_relaunch(cuda, name, form):
  r = _row('pair', name)
  _relaunch(r, cuda, lt.launch(r, lt.inputs(r), cuda, form=form)[1], form=form)


def test_pair_stats_refuses(cuda):
  r = _row('pair', 'n32m32-hw64')
  xd = lt.to_dev(lt.inputs(r), cuda)
  xd['a_t'] = xd['a'].transpose(0, 1).contiguous()
  bufs = lt.pair_buffers(r, cuda)
  for dims in [(33, 32, 64), (32, 33, 64), (32, 32, 62)]:
    _assert_refused(lambda: lt.pair_call(r, xd, bufs, dims=dims), bufs, lt.E_SHAPE, 'N, M, HW = %r' % (dims,))
  for strides in [(66, 3 * 64), (64, 3 * 64 + 2)]:
    _assert_refused(lambda: lt.pair_call(r, xd, bufs, tmajor=True, strides=strides), bufs, lt.E_SHAPE, 'strides %r' % (strides,))


# ---- ground-truth boxes, knobs, the rectangle IoU

@pytest.mark.parametrize('name', lt.names('box'))
def test_gt_box_knob_setup_box_iou_rects(cuda, name):
  """params against float64, box exactly (no corner lies within 1e-3 of a pixel index), ctr / size of the noisy boxes, the
  knob masks exactly, and the IoU of a map against the rectangles."""
  _parity(_row('box', name), cuda)


@pytest.mark.parametrize('name', ['40x36-b5t13', '9x4-b2t9', '64x68-b2t9'])
def test_gt_box_knob_setup_box_iou_rects_relaunch(cuda, name):
  r = _row('box', name)
  _relaunch(r, cuda, lt.launch(r, lt.inputs(r), cuda)[1])


def test_box_kernels_refuse(cuda):
  import ra_native as rn
  r = _row('box', '40x36-b2t17')
  xd = lt.to_dev(lt.inputs(r), cuda)
  bufs = lt.box_buffers(r, cuda)
  v, x = lambda k: rn.ptr(bufs[k].view), lambda k: rn.ptr(xd[k])
  B, T, H, W = r.p['B'], r.p['T'], r.p['H'], r.p['W']
  # H W = 34 * 35 is no multiple of 4 (the same pixels read as another shape: nothing is launched)
  _assert_refused(lambda: rn.lib().ra_gt_box_f32(x('y_gt'), B, T, 34, 35, lt.BOX_PAD_RATIO, lt.BOX_MIN_PAD, v('gt_ws'), B * T * 40, v('params'), v('box'),
                                                 rn.stream_ptr()), bufs, lt.E_SHAPE, 'H W % 4')
  _assert_refused(lambda: rn.lib().ra_gt_box_f32(x('y_gt'), B, T, H, W, lt.BOX_PAD_RATIO, lt.BOX_MIN_PAD, v('gt_ws'), B * T * 40 - 1, v('params'), v('box'),
                                                 rn.stream_ptr()), bufs, rn.RA_E_WORKSPACE, 'a short workspace')
  ws = bufs['rect_ws']
  # T = 33 rectangles of the 34 the row has; W = 34 is no multiple of 4
  _assert_refused(lambda: rn.lib().ra_box_iou_rects_f32(x('map'), v('params'), 1, 33, H, W, rn.ptr(ws), ws.numel(), v('iou'), rn.stream_ptr()), bufs,
                  lt.E_SHAPE, 'T = 33')
  _assert_refused(lambda: rn.lib().ra_box_iou_rects_f32(x('map'), v('params'), B, T, 36, 34, rn.ptr(ws), ws.numel(), v('iou'), rn.stream_ptr()), bufs,
                  lt.E_SHAPE, 'W % 4')
