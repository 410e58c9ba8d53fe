"""Training the pre-stage fg_model on the device (ra_fg_train.FgTrainStep, csrc/ra_fg_loss.hip, fg_model_train.py) against
the float64 oracle of tests/fg_train_oracle.py.

Measured on an MI355X (profiles/fg_train.txt has the table per case): the kernel's error is 1.5e-7 .. 1.1e-6 of the largest
gradient, at most 2.8 x the float32 torch error of its case (one-class bce: 8e-4 .. 5e-3 for both, the eps inside the logarithm
against an ulp of p near 1); whole graph: loss pieces equal to 7 digits, gradient cosine 1.000000; optimizer steps at most 0.97
(momentum) and 2.89 (Adam) float32 ulps; the whole file runs in under 4 s."""
import functools
import os

import numpy as np
import pytest
import torch

import fg_model
import fg_model_eval
import fg_model_train
import fg_oracle as fo
import fg_train_oracle as fto
import ra_fg_train
import ra_ops as ops
from ra_native import RecAttendError

pytestmark = pytest.mark.gpu


def _dev(a):
  return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _one_hot(idx, n):
  return np.eye(n, dtype=np.float32)[idx]


# ------------------------------------------------------------------------------------------- 1. the loss-gradient kernel
NPIX = (2 * 6 * 10, 3 * 20 * 28)  # less than a workgroup and no multiple of 64; several workgroups with a ragged tail
HEAD_CASES = [(nsc, no, seg, npix) for nsc in (1, 3, 9, 16) for no in (0, 8) for seg in ('iou', 'bce') for npix in NPIX]


def head_inputs(nsc, no, npix, seed, fg=0.3):
  """Logits of scale 6 (probabilities reach both ends, so the eps inside the logarithms matters), y_gt binary (nsc == 1) or
  one-hot with about 30 % foreground, d_gt one-hot; float32 values."""
  rng = np.random.RandomState(seed)
  z = (rng.randn(npix, nsc + no) * 6).astype(np.float32)
  if nsc == 1:
    y = (rng.rand(npix, 1) < fg).astype(np.float32)
  else:
    y = _one_hot(np.where(rng.rand(npix) < fg, rng.randint(1, nsc, npix), 0), nsc)
  d = _one_hot(rng.randint(0, 8, npix), 8) if no else None
  return z, y, d


def _rel_err(got, ref):
  return float(np.abs(got - ref).max() / np.abs(ref).max())


@functools.lru_cache(maxsize=None)
def head_table():
  """case -> (z, y, d, float64 autograd gradient, max |error| / max |reference| of the same formulas in float32 torch on the
  CPU).  Computed once and shared."""
  out = {}
  for i, (nsc, no, seg, npix) in enumerate(HEAD_CASES):
    z, y, d = head_inputs(nsc, no, npix, 100 + i)
    ref = fto.loss_grad(z, y, d, nsc, no, seg)
    out[(nsc, no, seg, npix)] = (z, y, d, ref, _rel_err(fto.loss_grad_formulas(z, y, d, nsc, no, seg, torch.float32), ref))
  return out


def head_bound(case):
  """At most 4 x the float32 torch error of the case (the order of operations differs), and never worse than the worst
  float32 torch error of the table."""
  tab = head_table()
  return min(4.0 * tab[case][4], max(v[4] for v in tab.values()))


def run_head(z, y, d, nsc, no, seg):
  zt, yt, dt = _dev(z), _dev(y), _dev(d)
  sums = ops.fg_stat_sums(zt, yt, dt, nsc, no)
  dz, status = ops.fg_loss_backward(zt, yt, dt, nsc, no, seg, sums)
  return dz, status


@pytest.mark.parametrize('nsc,no,seg,npix', HEAD_CASES)
def test_loss_gradient_kernel_vs_float64(cuda, nsc, no, seg, npix):
  z, y, d, ref, e32 = head_table()[(nsc, no, seg, npix)]
  dz, status = run_head(z, y, d, nsc, no, seg)
  dz2, _ = run_head(z, y, d, nsc, no, seg)
  got = dz.cpu().numpy().astype(np.float64)
  err, bound = _rel_err(got, ref), head_bound((nsc, no, seg, npix))
  print('fg_loss_bwd nsc %2d no %d %s npix %4d: kernel %.3e  float32 torch %.3e  bound %.3e' % (nsc, no, seg, npix, err, e32, bound))
  assert int(status.cpu()[0]) == 0
  assert torch.equal(dz, dz2)  # no atomics: the same bits on every run
  assert np.isfinite(got).all() and err <= bound, (err, e32, bound)


@pytest.mark.parametrize('seg', ['iou', 'bce'])
@pytest.mark.parametrize('nsc', [1, 3])
def test_loss_gradient_kernel_without_foreground(cuda, nsc, seg):
  """no = 8 and an all-background batch: status[0] = 1, the orientation gradient is zero, the semantic gradient is still
  that of the foreground loss."""
  npix = NPIX[0]
  z, y, d = head_inputs(nsc, 8, npix, 7, fg=0.0)
  assert (y if nsc == 1 else y[:, 1:]).sum() == 0
  dz, status = run_head(z, y, d, nsc, 8, seg)
  got = dz.cpu().numpy().astype(np.float64)
  assert int(status.cpu()[0]) == 1
  assert (got[:, nsc:] == 0).all()
  zs = np.ascontiguousarray(z[:, :nsc])
  ref = fto.loss_grad(zs, y, None, nsc, 0, seg)
  if seg == 'iou':  # I = 0 and g = 0 everywhere: -(g U - I (1 - g)) / U^2 is exactly zero
    assert (ref == 0).all() and (got[:, :nsc] == 0).all()
    return
  e32 = _rel_err(fto.loss_grad_formulas(zs, y, None, nsc, 0, seg, torch.float32), ref)
  err = _rel_err(got[:, :nsc], ref)
  print('fg_loss_bwd without foreground nsc %d %s: kernel %.3e  float32 torch %.3e' % (nsc, seg, err, e32))
  assert err <= 4.0 * e32


# --------------------------------------------------------------------------------- 2. the whole graph against float64 autograd
NETS = [(1, True), (3, True), (3, False)]
B, H, W = 2, 16, 24
DRAWS = dict(off_y=1, off_x=3)


def graph_opt(nsc, orientation, seg, **kw):
  return dict(fo.reduced_opt(nsc=nsc, orientation=orientation), padding=2, segm_loss_fn=seg, rnd_hflip=False, rnd_vflip=False,
              rnd_transpose=False, rnd_colour=False, base_learn_rate=1e-3, learn_rate_decay=0.96, steps_per_learn_rate_decay=5000,
              optimizer='adam', **kw)


def graph_batch(nsc, orientation, seed, n=B, fg=0.4):
  rng = np.random.RandomState(seed)
  x = rng.rand(n, H, W, 3).astype(np.float32)
  if nsc == 1:
    y = (rng.rand(n, H, W) < fg).astype(np.float32)
  else:
    y = _one_hot(np.where(rng.rand(n, H, W) < fg, rng.randint(1, nsc, (n, H, W)), 0), nsc)
  d = _one_hot(rng.randint(0, 8, (n, H, W)), 8) if orientation else None
  return x, y, d


@functools.lru_cache(maxsize=None)
def graph_reference(nsc, orientation, seg):
  opt = graph_opt(nsc, orientation, seg)
  P = fo.random_weights(opt, 11 + nsc)
  x, y, d = graph_batch(nsc, orientation, 21 + nsc)
  return opt, P, (x, y, d), fto.train_graph(opt, P, x, y, d, draws=DRAWS)


def _pre_bn_bias(name, opt):
  """A conv bias that feeds straight into BatchNorm: its true gradient is exactly zero."""
  nd = len(opt['dcnn_depth'])
  return name.endswith('/b') and name != 'dcnn/layer_%d/b' % (nd - 1)


def compare_grads(gref, got_of, opt):
  """The training step's own bars (tests/test_train_gpu.py): per tensor max |error| within 5 % of the tensor's largest
  gradient (or of 1e-3 of the largest gradient of all), the cosine over all gradients at least 0.9995; the biases in front
  of a BatchNorm have a zero gradient and must stay below 2e-3 of the scale."""
  dots, worst = np.zeros(3), {}
  gscale = max(np.abs(g).max() for g in gref.values())
  for k, g in gref.items():
    got = got_of(k)
    if _pre_bn_bias(k, opt):
      assert np.abs(got).max() < 2e-3 * gscale, k
      continue
    dots += [float((got * g).sum()), float((got * got).sum()), float((g * g).sum())]
    worst[k] = float(np.abs(got - g).max() / max(np.abs(g).max(), 1e-3 * gscale))
  cos = dots[0] / np.sqrt(dots[1] * dots[2])
  return cos, worst


@pytest.mark.parametrize('seg', ['iou', 'bce'])
@pytest.mark.parametrize('nsc,orientation', NETS)
def test_whole_graph_vs_float64_autograd(cuda, nsc, orientation, seg):
  opt, P, (x, y, d), ref = graph_reference(nsc, orientation, seg)
  model = fg_model.get_model(opt).load_weights(P)
  names = fg_model.save_var_names(model)
  ts = ra_fg_train.FgTrainStep(model)
  ts.bucket.zero_grad()
  loss, pieces, stats = ts.forward_loss(_dev(x), _dev(y), _dev(d), draws=DRAWS)
  loss.backward()
  assert np.array_equal(pieces['x_trans'].cpu().numpy(), ref['x_trans'].astype(np.float32))
  assert np.array_equal(pieces['y_gt_trans'].cpu().numpy().reshape(ref['y_gt_trans'].shape), ref['y_gt_trans'].astype(np.float32))
  if orientation:
    assert np.array_equal(pieces['d_gt_trans'].cpu().numpy(), ref['d_gt_trans'].astype(np.float32))
  assert set(ref['pieces']) == set(k for k in ra_fg_train.FETCHES if k in pieces)
  for k, v in ref['pieces'].items():
    print('%-16s %.8g (oracle %.8g)' % (k, float(pieces[k]), v))
    assert abs(float(pieces[k]) - v) < 2e-4 * max(1.0, abs(v)), k
  assert abs(float(loss.detach()) - ref['pieces']['loss']) < 2e-4 * max(1.0, abs(ref['pieces']['loss']))
  # batch moments and EMA shadows
  assert set(stats) == set(names[pre + '/bn/gamma'][:-len('_gamma')] for pre in ref['moments'])
  for pre, (mean, var) in ref['moments'].items():
    key = names[pre + '/bn/gamma'][:-len('_gamma')]
    for got, want, what in ((stats[key][0], mean, 'mean'), (stats[key][1], var, 'var'),
                            (model[key + '_ema_mean'], ref['ema'][pre + '/bn/ema_mean'], 'ema_mean'),
                            (model[key + '_ema_var'], ref['ema'][pre + '/bn/ema_var'], 'ema_var')):
      e = np.abs(got.cpu().numpy() - want).max() / max(1.0, np.abs(want).max())
      assert e < 1e-5, (pre, what, e)
  # every parameter gradient; the device leaves wd * w to the optimizer kernel
  cos, worst = compare_grads(ref['data_grads'], lambda k: ts.bucket.grad_of[names[k]].cpu().numpy().astype(np.float64), opt)
  print('gradient cosine %.6f, worst per-tensor relative error %.4f (%s)' % (cos, max(worst.values()), max(worst, key=worst.get)))
  bad = {k: v for k, v in worst.items() if v > 5e-2}
  assert cos >= 0.9995 and not bad, (cos, sorted(bad.items(), key=lambda kv: -kv[1])[:8])


# --------------------------------------------------------------------------------------------------- 3. the optimizer steps
def _ulps(got, ref, scale):
  """|got - ref| in float32 ulps of `scale`, elementwise."""
  return np.abs(got.astype(np.float64) - ref) / np.spacing(np.maximum(np.abs(scale), np.finfo(np.float32).tiny).astype(np.float32)).astype(np.float64)


@pytest.mark.parametrize('optimizer', ['momentum', 'adam'])
def test_optimizer_step_vs_float64(cuda, optimizer):
  """One step from the device's own gradients against a float64 restatement of the update with the float32 values the kernel is
  handed (lr, the betas, wd): 4 float32 ulps of max(|p|, |lr * accum|) per element — three roundings and a possible FMA
  contraction.  Then a second step from the slots of the first: the terms that are added into a slot may now cancel, and
  the slot's rounding error (in ulps of its largest term) reaches the update undiminished, so the second step's scale is the
  update that the largest term alone would make."""
  opt = graph_opt(3, True, 'bce', weight_decay=5e-5)
  opt['optimizer'] = optimizer
  opt['base_learn_rate'] = 1e-2 if optimizer == 'momentum' else 1e-3
  model = fg_model.get_model(opt).load_weights(fo.random_weights(opt, 5))
  ts = ra_fg_train.FgTrainStep(model)
  x, y, d = (_dev(a) for a in graph_batch(3, True, 6))
  b = ts.bucket
  f4 = lambda v: float(np.float32(v))
  slots = [np.zeros(b.n), np.zeros(b.n)]
  for step in range(2):
    p0 = b.param.cpu().numpy().astype(np.float64)
    out = ts.run(x, y, d, draws=DRAWS)
    grad, decay = b.grad.cpu().numpy().astype(np.float64), b.wd.cpu().numpy().astype(np.float64) * p0
    g = grad + decay
    gmax = np.maximum(np.abs(grad), np.abs(decay))  # grad and wd * p may cancel: g is exact to an ulp of the larger of the two
    lr = f4(out['learn_rate'])
    if optimizer == 'momentum':
      want, acc = fto.momentum_step(p0, g, slots[0], lr, momentum=f4(0.9))
      upd = lr * acc
      reach = lr * np.maximum(np.abs(f4(0.9) * slots[0]), gmax)
      # the slot: 4 ulps of the largest term that is added (they may cancel)
      assert _ulps(ts.accum.cpu().numpy(), acc, np.maximum(np.abs(f4(0.9) * slots[0]), gmax)).max() <= 4
    else:
      t = step + 1
      lr_t = f4(out['learn_rate'] * np.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t))
      b1, b2, eps = f4(0.9), f4(0.999), f4(1e-7)
      m = b1 * slots[0] + (1 - b1) * g
      v = b2 * slots[1] + (1 - b2) * g * g
      upd = lr_t * m / (np.sqrt(v) + eps)
      want = p0 - upd
      reach = lr_t * np.maximum(np.abs(b1 * slots[0]), (1 - b1) * gmax) / (np.sqrt(v) + eps)
      # the slots, likewise; in v an ulp of gmax on g is 2 |g| ulp(gmax) <= 4 ulps of gmax^2 on g^2, plus three roundings
      assert _ulps(b.m.cpu().numpy(), m, np.maximum(np.abs(b1 * slots[0]), (1 - b1) * gmax)).max() <= 4
      assert _ulps(b.v.cpu().numpy(), v, np.maximum(b2 * slots[1], (1 - b2) * gmax * gmax)).max() <= 8
    scale = np.maximum(np.abs(p0), np.abs(upd))
    u = _ulps(b.param.cpu().numpy(), want, scale if step == 0 else np.maximum(scale, reach))
    print('%s step %d: worst %.2f float32 ulps of max(|p|, |update|%s)' % (optimizer, step, u.max(), '' if step == 0 else ', |reach|'))
    assert u.max() <= 4
    # continue from the device's own slots, so that the second step checks one update, not two
    slots = [ts.accum.cpu().numpy().astype(np.float64), None] if optimizer == 'momentum' else \
        [b.m.cpu().numpy().astype(np.float64), b.v.cpu().numpy().astype(np.float64)]
  assert b.global_step == 2 and model['global_step'] == 2.0


def test_learn_rate_staircase_and_global_step(cuda):
  opt = graph_opt(1, True, 'iou')
  opt.update(steps_per_learn_rate_decay=2, learn_rate_decay=0.5, base_learn_rate=2e-3)
  ts = ra_fg_train.FgTrainStep(fg_model.get_model(opt).load_weights(fo.random_weights(opt, 5)))
  x, y, d = (_dev(a) for a in graph_batch(1, True, 6))
  rates = [ts.run(x, y, d)['learn_rate'] for _ in range(5)]
  ts.flush_status()
  assert rates == pytest.approx([fto.learn_rate(opt, s) for s in range(5)], rel=1e-15) and rates[2] == pytest.approx(1e-3)
  assert ts.bucket.global_step == 5


@pytest.mark.parametrize('optimizer', ['momentum', 'adam'])
def test_step_without_foreground_is_skipped(cuda, optimizer):
  opt = graph_opt(3, True, 'bce')
  opt['optimizer'] = optimizer
  ts = ra_fg_train.FgTrainStep(fg_model.get_model(opt).load_weights(fo.random_weights(opt, 5)))
  x, y, d = graph_batch(3, True, 6)
  ts.run(_dev(x), _dev(y), _dev(d))  # a good step first: the slots are not all zero
  ts.flush_status()
  keep = [t.clone() for t in (ts.bucket.param, ts.accum, ts.bucket.m, ts.bucket.v)]
  y0 = np.zeros_like(y)
  y0[..., 0] = 1
  out = ts.run(_dev(x), _dev(y0), _dev(d))
  assert np.isnan(float(out['orientation_ce'])) and np.isnan(float(out['loss']))  # the reference's 0 / 0
  for a, t in zip(keep, (ts.bucket.param, ts.accum, ts.bucket.m, ts.bucket.v)):
    assert torch.equal(a, t)
  assert ts.bucket.global_step == 2
  with pytest.raises(RecAttendError, match='no foreground pixel'):
    ts.flush_status()
  assert ts.bucket.global_step == 1  # the skipped step's number is given back
  ts.run(_dev(x), _dev(y), _dev(d))
  ts.flush_status()
  assert ts.bucket.global_step == 2 and not torch.equal(keep[0], ts.bucket.param)


# ------------------------------------------------------------------------------------------------------------- 4. it trains
@pytest.mark.parametrize('optimizer,lr', [('adam', 1e-3), ('momentum', 1e-2)])
def test_five_steps_on_one_batch(cuda, optimizer, lr):
  opt = graph_opt(3, True, 'bce')
  opt.update(optimizer=optimizer, base_learn_rate=lr, padding=0)
  model = fg_model.get_model(opt).load_weights(fo.random_weights(opt, 31))
  ts = ra_fg_train.FgTrainStep(model)
  shadows = {k: model[k].clone() for k in model if isinstance(k, str) and k.endswith(('_ema_mean', '_ema_var'))}
  x, y, d = (_dev(a) for a in graph_batch(3, True, 32))
  losses = [float(ts.run(x, y, d)['loss']) for _ in range(5)]
  ts.flush_status()
  print('%s: losses %s' % (optimizer, ' '.join('%.5f' % v for v in losses)))
  assert np.isfinite(losses).all() and losses[-1] < losses[0]
  assert shadows and all(not torch.equal(v, model[k]) for k, v in shadows.items())
  # the eval closures see the trained weights after sync_model()
  before = model.statistics(x, y, d)
  ts.sync_model()
  after = model.statistics(x, y, d)
  assert np.isfinite(after['loss']) and after['loss'] != before['loss']


# -------------------------------------------------------------------------------------------------------------- 5. the chain
def test_train_pack_eval_chain(cuda, tmp_path, capsys):
  rng = np.random.RandomState(41)
  n = 4
  x, y, d = graph_batch(1, True, 42, n=n)
  src = str(tmp_path / 'train.npz')
  np.savez(src, x=x, y_gt=y, d_gt=d, fg_gt_full=(rng.rand(n, 2 * H, 2 * W) < 0.4).astype(np.uint8))
  res = str(tmp_path / 'results')
  net = ('--cnn_depth 8,16,16,24,24 --cnn_pool 1,2,1,2,1 --cnn_skip_mask 1,0,1,0,1 --dcnn_depth 16,16,12,8,9 --dcnn_pool 1,2,1,2,1 '
         '--dcnn_skip_mask 1,1,0,1 --add_skip_conn --add_orientation --segm_loss_fn bce --optimizer momentum --padding 2').split()
  common = net + ['--model_id', 'fg', '--results', res, '--input', src, '--batch_size', '2', '--steps_per_log', '1']
  tr = fg_model_train.main(common + ['--num_steps', '3', '--save_ckpt', '--steps_per_ckpt', '2', '--valid_input', src, '--steps_per_valid', '2'])
  assert tr.bucket.global_step == 3
  folder = os.path.join(res, 'fg')
  assert sorted(os.listdir(folder)) == ['log.txt', 'model_opt.yaml', 'optimizer.npz', 'weights.npz']
  log = open(os.path.join(folder, 'log.txt')).read().splitlines()
  assert [l.split()[:2] for l in log[:3]] == [['step', '0'], ['step', '1'], ['step', '1']] and 'valid' in log[2]
  import yaml
  with open(os.path.join(folder, 'model_opt.yaml')) as f:
    opt = yaml.safe_load(f)
  weights = dict(np.load(os.path.join(folder, 'weights.npz')))
  assert float(weights['step']) == 3.0
  model = fg_model.get_model(opt).load_weights(weights)  # strict
  assert sorted(weights) == sorted(list(fg_model.save_var_names(model)) + ['step'])
  for k, v in tr.model.state_dict_numpy().items():
    assert np.array_equal(weights[k], v), k
  out = fg_model_eval.main(['--model_id', 'fg', '--results', res, '--input', src, '--output', str(tmp_path / 'eval'), '--batch_size', '2'])
  assert set(out['statistics']) == {'iou_soft', 'iou_hard', 'foreground_loss', 'loss', 'orientation_ce', 'orientation_acc'}
  assert all(np.isfinite(v) for v in out['statistics'].values())
  # --restore: the same optimizer state, and the run goes on at step 3
  state = dict(np.load(os.path.join(folder, 'optimizer.npz')))
  assert int(state['global_step']) == 3 and any(k.startswith('momentum/') for k in state) and any(k.startswith('adam_m/') for k in state)
  tr2 = fg_model_train.main(['--model_id', 'fg2', '--results', res, '--input', src, '--batch_size', '2', '--restore', folder,
                             '--num_steps', '3'])
  got = tr2.state_dict()
  assert sorted(got) == sorted(state) and all(np.array_equal(got[k], state[k]) for k in state)
  assert all(np.array_equal(v, weights[k]) for k, v in tr2.model.state_dict_numpy().items())
  capsys.readouterr()
  tr3 = fg_model_train.main(['--model_id', 'fg2', '--results', res, '--input', src, '--batch_size', '2', '--restore', folder,
                             '--num_steps', '4', '--steps_per_log', '1'])
  text = capsys.readouterr().out
  assert 'restored' in text and 'global_step 3' in text and '\nstep 3 ' in text and '\nstep 2 ' not in text
  assert tr3.bucket.global_step == 4
