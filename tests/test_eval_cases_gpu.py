"""Float64 parity of the evaluator's kernels (csrc/ra_eval.hip) over their dimension space, through the C ABI:
ra_postprocess_f32, ra_union_f32, ra_weighted_sum_f32, ra_remove_tiny_f32, ra_dilate_f32, ra_resize_linear_f32,
ra_bilateral5_f32 (and utils/postprocess.upsample), ra_eval_metrics_f32 (and ra_ops.eval_metrics on masks),
ra_random_transform_f32 and ra_colour_jitter_f32.

The rows, the references and the bars are in tests/eval_cases.py; tests/test_eval_cases.py asserts on the host that the float32
CPU run of every reference sits 8 times inside every bar used here, that no input sits where float32 and float64 could disagree
on a discrete output, and that the rows reach the launch choices they were chosen for.  Every output lies in a buffer of sentinel
words and starts as NaN (the jitter's workspace too), so a hole or a write outside is seen whatever a previous launch left in
memory; no pixel or element is left out of a comparison.  Per family: every row against float64, a launch into buffers another
draw has filled giving the bits of a launch into fresh ones, and the refused calls with their code and their outputs untouched."""
import numpy as np
import pytest

import eval_cases as ec

pytestmark = pytest.mark.gpu


def _assert_scores(scores, what):
  bad = []
  assert scores, what
  for w, e, bar in scores:
    print('%s %s: %.3g (bar %g)' % (what, w, e, bar))
    if not e < bar:
      bad.append((w, e, bar))
  assert not bad, '%s: %s' % (what, bad)


def _row(family, name):
  return ec.ROW_OF[(family, name)]


def _parity(r, cuda):
  bufs, got = ec.launch(r, ec.inputs(r), cuda)
  _assert_scores(ec.scores(r, ec.reference(r), got), '%s %s' % (r.family, r.name))
  return bufs, got


def _bytes(got):
  return b''.join(np.ascontiguousarray(got[k]).tobytes() for k in sorted(got))


def _relaunch(r, cuda):
  """Another draw of the inputs into new buffers, then the row's own into the same ones: the bits of a launch into fresh ones."""
  fresh = ec.launch(r, ec.inputs(r), cuda)[1]
  bufs, other = ec.launch(r, ec.inputs(r, alt=True), cuda)
  assert bufs and _bytes(other) != _bytes(fresh), 'the other draw gave the same results: the relaunch shows nothing'
  _, again = ec.launch(r, ec.inputs(r), cuda, bufs=bufs)
  for k in fresh:
    assert np.ascontiguousarray(again[k]).tobytes() == np.ascontiguousarray(fresh[k]).tobytes(), (r.name, k)


def _refused(r, cuda):
  """The call returns its code without a launch: the guarded buffers keep every bit."""
  import ra_native as rn
  call, bufs, code = ec.refused(r, cuda)
  guarded = ec.guarded_only(bufs)
  assert guarded
  before = ec.bits_of(guarded)
  rc = call()
  assert rc == code, '%s: returned %d, not %d (%s)' % (r.name, rc, code, (rn.lib().ra_last_error_string() or b'').decode())
  assert ec.bits_of(guarded) == before, '%s: a refused call wrote to its outputs' % r.name


def _rejected(family):
  return pytest.mark.parametrize('r', ec.REJECTED[family], ids=[r.name for r in ec.REJECTED[family]])


# ---- post-processing

@pytest.mark.parametrize('name', ec.names('post'))
def test_postprocess(cuda, name):
  """y_bin, s_hard and the union exactly: the first maximum on a full-T tie, strict > on the threshold, -inf as apply_one_label passes it."""
  _parity(_row('post', name), cuda)


@pytest.mark.parametrize('name', ['hw1028-b1t256-fg-uni-half', 'hw1020-b3t5-nofg-uni-ninf'])
def test_postprocess_relaunch(cuda, name):
  _relaunch(_row('post', name), cuda)


@_rejected('post')
def test_postprocess_refuses(cuda, r):
  _refused(r, cuda)


@pytest.mark.parametrize('name', ec.names('union'))
def test_union(cuda, name):
  _parity(_row('union', name), cuda)


def test_union_relaunch(cuda):
  _relaunch(_row('union', 'hw1028-t5'), cuda)


@_rejected('union')
def test_union_refuses(cuda, r):
  _refused(r, cuda)


@pytest.mark.parametrize('name', ec.names('wsum1'))
def test_weighted_sum(cuda, name):
  """A zero weight's plane holds an inf: the term is skipped, not multiplied; an image of zero weights is 0 bit for bit."""
  _parity(_row('wsum1', name), cuda)


@pytest.mark.parametrize('name', ['hw1028-t5-zeros', 'hw1020-t32-general'])
def test_weighted_sum_relaunch(cuda, name):
  _relaunch(_row('wsum1', name), cuda)


@_rejected('wsum1')
def test_weighted_sum_refuses(cuda, r):
  _refused(r, cuda)


@pytest.mark.parametrize('name', ec.names('tiny'))
def test_remove_tiny(cuda, name):
  """In place: a plane of exactly `threshold` is removed, one above is kept bit for bit; conf follows, or is null."""
  _parity(_row('tiny', name), cuda)


@pytest.mark.parametrize('name', ['hw16388-6-conf', 'hw8196-6-noconf'])
def test_remove_tiny_relaunch(cuda, name):
  _relaunch(_row('tiny', name), cuda)


@_rejected('tiny')
def test_remove_tiny_refuses(cuda, r):
  _refused(r, cuda)


@pytest.mark.parametrize('name', ec.names('dilate'))
def test_dilate(cuda, name):
  _parity(_row('dilate', name), cuda)


@pytest.mark.parametrize('name', ['16x17-r16-real', '2x130-r2-bin'])
def test_dilate_relaunch(cuda, name):
  _relaunch(_row('dilate', name), cuda)


@_rejected('dilate')
def test_dilate_refuses(cuda, r):
  _refused(r, cuda)


@pytest.mark.parametrize('name', ec.names('resize'))
def test_resize_linear(cuda, name):
  """Non-integer ratios up and down, 1 x 1 and 1 x N sources, a 1 x 1 result; at equal size a copy bit for bit."""
  _parity(_row('resize', name), cuda)


@pytest.mark.parametrize('name', ['5x7-13x16', '2x2-64x64'])
def test_resize_linear_relaunch(cuda, name):
  _relaunch(_row('resize', name), cuda)


@pytest.mark.parametrize('name', ec.names('bilateral'))
def test_bilateral5(cuda, name):
  """Planes below the window's size (reflect101 at n = 1, 2, 3), a small sigma_color; two rows through utils/postprocess.upsample."""
  _parity(_row('bilateral', name), cuda)


@pytest.mark.parametrize('name', ['16x17-sc0.1-bin', '2x2-sc10-smooth'])
def test_bilateral5_relaunch(cuda, name):
  _relaunch(_row('bilateral', name), cuda)


@_rejected('bilateral')
def test_bilateral5_refuses(cuda, r):
  _refused(r, cuda)


# ---- metrics

@pytest.mark.parametrize('name', ec.names('metrics'))
def test_eval_metrics(cuda, name):
  """Constructed integer tables: images without ground truth, without outputs, with count_gt = T; both-empty pairs; IoU 1/2
  exactly and 499/999 under the >= 0.5 flags; every nullable pointer null in turn; three rows through ra_ops.eval_metrics on masks."""
  _parity(_row('metrics', name), cuda)


@pytest.mark.parametrize('name', ['b2t32', 'b3t5'])
def test_eval_metrics_relaunch(cuda, name):
  _relaunch(_row('metrics', name), cuda)


@_rejected('metrics')
def test_eval_metrics_refuses(cuda, r):
  _refused(r, cuda)


# ---- the in-graph augmentation

@pytest.mark.parametrize('name', ec.names('transform'))
def test_random_transform(cuda, name):
  _parity(_row('transform', name), cuda)


@pytest.mark.parametrize('name', ['16x16x9-p3-far-v1h0t1', '5x7x3-allpad-v0h1t0'])
def test_random_transform_relaunch(cuda, name):
  r = _row('transform', name)
  if 'allpad' in name:  # all zeros whatever the input: the relaunch is into buffers a crop of the other draw has filled
    bufs, other = ec.launch(_row('transform', '5x7x3-p3-mid-v0h1t0'), ec.inputs(r, alt=True), cuda)
    assert np.abs(other['out']).max() > 0
    fresh = ec.launch(r, ec.inputs(r), cuda)[1]
    again = ec.launch(r, ec.inputs(r), cuda, bufs=bufs)[1]
    assert again['out'].tobytes() == fresh['out'].tobytes()
  else:
    _relaunch(r, cuda)


@_rejected('transform')
def test_random_transform_refuses(cuda, r):
  _refused(r, cuda)


@pytest.mark.parametrize('name', ec.names('jitter'))
def test_colour_jitter(cuda, name):
  """The workspace starts as NaN: every partial-sum record is written, by the workgroups without a pixel too; grey, black, white
  and pure-primary pixels; the identity draws."""
  _parity(_row('jitter', name), cuda)


@pytest.mark.parametrize('name', ['hw40000-b3-corner2', 'hw1-b3-corner1'])
def test_colour_jitter_relaunch(cuda, name):
  _relaunch(_row('jitter', name), cuda)


@_rejected('jitter')
def test_colour_jitter_refuses(cuda, r):
  _refused(r, cuda)
