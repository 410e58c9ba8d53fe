"""Training the pre-stage fg_model, the parts that need no device: the trainer's refusals, the float64 oracle of the training
graph (tests/fg_train_oracle.py) against the eval oracle's statistics and against itself (closed-form gradient of the loss
head against autograd), the argument checks of the new entry points, and the command line against the reference's
fg_model_train.py:425-448."""
import numpy as np
import pytest
import torch

import fg_eval_oracle as fe
import fg_model
import fg_model_train
import fg_oracle as fo
import fg_train_oracle as fto
import ra_fg_train
import ra_native as rn
from ra_native import RecAttendError


# ---- 1. refusals, all in the constructor, none of which needs a device
def _trainer(opt):
  return ra_fg_train.FgTrainStep(fg_model.get_model(opt))


@pytest.mark.parametrize('opt', [fo.reduced_opt(wide=True), fo.kitti_opt()], ids=['reduced-wide', 'kitti'])
def test_wide_nets_are_refused(opt):
  with pytest.raises(RecAttendError, match='training with layers of .* output channels is not built .*eval decodes'):
    _trainer(opt)


def test_option_refusals():
  opt = fo.reduced_opt()
  with pytest.raises(RecAttendError, match='dcnn_filter_size .* is not built'):
    _trainer(dict(opt, dcnn_filter_size=[3, 5, 3, 3, 3]))
  with pytest.raises(RecAttendError, match='segm_loss_fn'):
    _trainer(dict(opt, segm_loss_fn='wt_cov'))
  with pytest.raises(RecAttendError, match='optimizer'):
    _trainer(dict(opt, optimizer='sgd'))
  for flag in ('rnd_hflip', 'rnd_vflip', 'rnd_transpose'):
    with pytest.raises(RecAttendError, match='orientation mode, %s not supported' % flag):
      _trainer(dict(opt, **{flag: True}))


def test_several_ranks_are_refused(monkeypatch):
  monkeypatch.setenv('WORLD_SIZE', '2')
  with pytest.raises(RecAttendError, match='WORLD_SIZE'):
    _trainer(fo.reduced_opt())


def test_no_device_is_refused(monkeypatch):
  monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
  monkeypatch.delenv('WORLD_SIZE', raising=False)
  with pytest.raises(RecAttendError, match='needs an MI355X'):
    _trainer(fo.reduced_opt(nsc=3, orientation=False))


def test_kernel_forms_of_the_run_script_channel_counts():
  """9, 11, 12, 17 and 24 outputs and a 3-channel skip source pass the kernels' own host-side checks; a count K1 has no
  form for is named by the constructor's check."""
  for nsc, ori in ((1, True), (3, True), (9, True), (3, False)):
    ra_fg_train.check_kernel_forms(fg_model.derive(fo.reduced_opt(nsc=nsc, orientation=ori)))
  d = fg_model.derive(fo.reduced_opt())
  d['cnn_channels'][2] = 130
  with pytest.raises(RecAttendError, match='cnn layer 1'):
    ra_fg_train.check_kernel_forms(d)
  # the command line's default net with its skips: dcnn layer 2 reads 128 + 64 channels, and its data gradient is a conv of
  # 192 outputs; with that layer's predecessor at 64 channels every input fits
  p = fg_model_train.build_parser()
  flags = ['--add_skip_conn', '--add_orientation', '--dcnn_depth']
  opt = fg_model_train.make_opt(p.parse_args(flags + ['128,128,64,64,32,32,16,16,8,8,9']))
  with pytest.raises(RecAttendError, match='dcnn layer 2 .*192 channels is not built'):
    ra_fg_train.check_kernel_forms(fg_model.derive(opt))
  with pytest.raises(RecAttendError, match='dcnn layer 2 .*192 channels is not built'):
    _trainer(opt)
  ra_fg_train.check_kernel_forms(fg_model.derive(fg_model_train.make_opt(p.parse_args(flags + ['128,64,64,64,32,32,16,16,8,8,9']))))


# ---- 2. the oracle: its loss against the eval oracle's statistics, its closed forms against its autograd
def _head_case(nsc, no, npix, seed, fg=0.3):
  rng = np.random.RandomState(seed)
  z = rng.randn(npix, nsc + no) * 6
  if nsc == 1:
    y = (rng.rand(npix, 1) < fg).astype(np.float64)
  else:
    cls = np.where(rng.rand(npix) < fg, rng.randint(1, nsc, npix), 0)
    y = np.eye(nsc)[cls]
  d = np.eye(8)[rng.randint(0, 8, npix)] if no else None
  return z, y, d


@pytest.mark.parametrize('seg', ['iou', 'bce'])
@pytest.mark.parametrize('nsc,no', [(1, 0), (1, 8), (3, 8), (9, 8), (16, 0)])
def test_oracle_loss_and_gradient(nsc, no, seg):
  z, y, d = _head_case(nsc, no, 2 * 6 * 10, 7 + nsc)
  t = lambda a: None if a is None else torch.from_numpy(a)
  got = {k: float(v) for k, v in fto.loss_pieces(t(z), t(y), t(d), nsc, no, seg).items()}
  want = fe.statistics(z, y, d, nsc, no, seg)
  assert set(got) == set(want)
  for k in want:
    assert abs(got[k] - want[k]) <= 1e-12 * max(1.0, abs(want[k])), (k, got[k], want[k])
  ref = fto.loss_grad(z, y, d, nsc, no, seg)
  closed = fto.loss_grad_formulas(z, y, d, nsc, no, seg, dtype=torch.float64)
  # p + eps and 1 - p + eps: p carries half an ulp of 1 (2^-53), the sum is at least eps = 1e-5, so a quotient is off by up to
  # 2^-53 / 1e-5 = 1.1e-11 of itself; a handful of such terms per element
  assert np.abs(closed - ref).max() <= 1e-10 * np.abs(ref).max()
  # the same in float32: 2^-24 / 1e-5 = 6e-3 of an element, on elements no larger than the largest
  f32 = fto.loss_grad_formulas(z, y, d, nsc, no, seg, dtype=torch.float32)
  assert np.abs(f32 - ref).max() <= 2e-2 * np.abs(ref).max()


def test_oracle_graph_matches_the_eval_oracle_at_its_own_moments():
  """The training graph's logits equal the eval oracle's when the shadows hold the batch moments: the two restatements of
  the stack pin each other."""
  opt = dict(fo.reduced_opt(nsc=3, orientation=True), padding=2, segm_loss_fn='bce')
  P = fo.random_weights(opt, 3)
  rng = np.random.RandomState(4)
  x = rng.rand(2, 16, 24, 3)
  z, y, d = _head_case(3, 8, 2 * 16 * 24, 5)
  out = fto.train_graph(opt, P, x, y.reshape(2, 16, 24, 3), d.reshape(2, 16, 24, 8), draws=dict(off_y=1, off_x=3))
  assert out['x_trans'].shape == x.shape and (out['x_trans'][:, 1:, :-1] == x[:, :-1, 1:]).all() and (out['x_trans'][:, 0] == 0).all()
  Q = dict(P)
  for pre, (mean, var) in out['moments'].items():
    Q[pre + '/bn/ema_mean'], Q[pre + '/bn/ema_var'] = mean, var
  ev = fo.forward(opt, Q, out['x_trans'])
  assert np.abs(ev['logits'] - out['logits']).max() <= 1e-9 * np.abs(out['logits']).max()
  st = fe.statistics(out['logits'], out['y_gt_trans'], out['d_gt_trans'], 3, 8, 'bce')
  for k, v in st.items():
    assert abs(out['pieces'][k] - v) <= 1e-12 * max(1.0, abs(v)), k
  # wd * l2_loss(w) over the filters only
  l2 = sum(float((np.asarray(P[k], np.float64) ** 2).sum()) / 2 for k in P if k.endswith('/w'))
  assert abs(out['total_loss'] - out['pieces']['loss'] - opt['weight_decay'] * l2) <= 1e-12
  k = 'dcnn/layer_1/w'
  assert np.allclose(out['grads'][k], out['data_grads'][k] + opt['weight_decay'] * np.asarray(P[k], np.float64), rtol=0, atol=1e-15)
  assert np.array_equal(out['grads']['cnn/layer_0/b'], out['data_grads']['cnn/layer_0/b'])


def test_oracle_optimizers():
  rng = np.random.RandomState(0)
  p, g = rng.randn(5), rng.randn(5)
  q, m, v = fto.adam_step(p, g, np.zeros(5), np.zeros(5), 1e-3, 1)
  assert np.allclose(q, p - 1e-3 * np.sign(g), rtol=1e-5)  # the first Adam step moves every parameter by lr
  q, a = fto.momentum_step(p, g, np.ones(5), 0.1)
  assert np.allclose(a, 0.9 + g) and np.allclose(q, p - 0.1 * (0.9 + g))
  opt = dict(base_learn_rate=0.5, learn_rate_decay=0.1, steps_per_learn_rate_decay=2)
  assert [fto.learn_rate(opt, s) for s in range(5)] == pytest.approx([0.5, 0.5, 0.05, 0.05, 0.005])


# ---- 3. the entry points refuse bad arguments before any launch (host pointers: nothing is dereferenced)
def test_entry_points_refuse_bad_arguments():
  lib = rn.lib()
  ok = dict(logits=1, y_gt=1, d_gt=1, npix=16, nsc=3, no=8, seg=0, sums=1, up=1.0, dl=1, status=1)

  def call(**kw):
    a = dict(ok, **kw)
    return lib.ra_fg_loss_bwd_f32(a['logits'], a['y_gt'], a['d_gt'], a['npix'], a['nsc'], a['no'], a['seg'], a['sums'], a['up'],
                                  a['dl'], a['status'], None)

  for bad in (dict(nsc=0), dict(nsc=17), dict(no=4), dict(seg=2), dict(seg=-1)):
    assert call(**bad) == rn.RA_E_SHAPE, bad
    assert b'ra_fg_loss_bwd_f32' in lib.ra_last_error_string()
  for bad in (dict(logits=None), dict(y_gt=None), dict(d_gt=None), dict(sums=None), dict(dl=None), dict(status=None), dict(npix=0)):
    assert call(**bad) == rn.RA_E_INVALID, bad
  mom = lambda p=1, g=1, a=1, status=1, n_status=1: lib.ra_momentum_step_guarded_f32(p, g, a, None, 8, 0.1, 0.9, 1.0, status, n_status, None)
  assert mom(p=None) == mom(g=None) == mom(a=None) == rn.RA_E_INVALID
  assert mom(status=None) == rn.RA_E_INVALID and mom(n_status=-1) == rn.RA_E_INVALID
  assert lib.ra_momentum_step_guarded_f32(1, 1, 1, None, 0, 0.1, 0.9, 1.0, None, 0, None) == 0  # nothing to do, nothing launched
  import ra_ops as ops
  z = torch.zeros(4, 9)
  with pytest.raises(RecAttendError, match='segm_loss_fn'):
    ops.fg_loss_backward(z, z[:, :1], z[:, 1:], 1, 8, 'mse', torch.zeros(9, dtype=torch.float64))
  with pytest.raises(RecAttendError, match='no CPU fallback'):
    ops.fg_loss_backward(z, z[:, :1].contiguous(), z[:, 1:].contiguous(), 1, 8, 'iou', torch.zeros(9, dtype=torch.float64))


# ---- 4. the command line against fg_model_train.py:425-448
def test_cli_defaults_and_parsing():
  p = fg_model_train.build_parser()
  a = p.parse_args([])
  want = dict(cnn_filter_size='3,3,3,3,3,3,3,3,3,3', cnn_depth='8,8,16,16,32,32,64,64,128,128', cnn_pool='1,2,1,2,1,2,1,2,1,2',
              dcnn_filter_size='3,3,3,3,3,3,3,3,3,3,3', dcnn_depth='128,128,64,64,32,32,16,16,8,8,1',
              dcnn_pool='2,1,2,1,2,1,2,1,2,1,1', add_skip_conn=False, cnn_skip_mask='1,0,0,0,0,0,1,0,1,0',
              dcnn_skip_mask='0,1,0,1,0,0,0,0,0,1', segm_loss_fn='iou', add_orientation=False, num_orientation_classes=8,
              num_semantic_classes=1, base_learn_rate=1e-3, learn_rate_decay=0.96, steps_per_learn_rate_decay=5000,
              rnd_colour=False, padding=16, optimizer='adam')
  for k, v in want.items():
    assert getattr(a, k) == v, k
  assert (a.model_id, a.results, a.num_steps, a.batch_size, a.steps_per_valid, a.save_ckpt, a.restore, a.seed, a.input,
          a.valid_input) == (None, 'results', 500000, 32, 50, False, None, 1234, None, None)
  opt = fg_model_train.make_opt(a)
  assert opt['cnn_filter_size'] == [3] * 10 and opt['dcnn_filter_size'] == [3] * 11 and opt['weight_decay'] == 5e-5
  assert opt['cnn_skip_mask'] == [True, False, False, False, False, False, True, False, True, False]
  assert (opt['rnd_hflip'], opt['rnd_vflip'], opt['rnd_transpose'], opt['use_bn']) == (False, False, False, True)
  assert (opt['inp_height'], opt['inp_width'], opt['inp_depth']) == (224, 224, 3)
  fg_model.derive(dict(opt, add_skip_conn=True))  # the default net is well-formed, and it stays within 128 channels
  # run_kitti.sh's fg flags
  a = p.parse_args('--dataset kitti --cnn_filter_size 5,5 --cnn_depth 8,16 --cnn_pool 1,2 --dcnn_depth 8,9 --dcnn_pool 2,1 '
                   '--add_skip_conn --cnn_skip_mask 1,0 --dcnn_skip_mask 1 --segm_loss_fn bce --add_orientation '
                   '--num_semantic_classes 1 --optimizer momentum --base_learn_rate 0.01 --padding 4 --rnd_colour '
                   '--model_id fg --num_steps 3 --batch_size 2 --save_ckpt --steps_per_valid 2'.split())
  opt = fg_model_train.make_opt(a)
  assert opt['cnn_filter_size'] == [3, 3] and opt['cnn_depth'] == [8, 16] and opt['dcnn_filter_size'] == [3, 3]
  assert (opt['inp_height'], opt['inp_width'], opt['optimizer'], opt['segm_loss_fn'], opt['padding'], opt['rnd_colour']) == \
      (128, 448, 'momentum', 'bce', 4, True)
  assert fg_model.derive(opt)['skip_src'] == [None, 0]
  with pytest.raises(Exception, match='model ID'):
    fg_model_train.main([])
  with pytest.raises(RecAttendError, match='--input'):
    fg_model_train.main(['--model_id', 'fg'])
