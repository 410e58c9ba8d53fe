"""Training the wide layers of fg_model on the device — FgTrainStep(model, wide=True), ra_fg_train.WideConvBNActPool, the device
pack of the wide conv — against the host pack, float64 autograd and the float64 oracle of tests/fg_train_oracle.py."""
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
from test_fg_train_gpu import DRAWS, _dev, compare_grads, graph_batch

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------------ 1. the device pack
def _filter(shape, seed):
  return np.random.RandomState(seed).randn(*shape).astype(np.float32)


@pytest.mark.parametrize('transposed', [False, True])
def test_device_pack_equals_host_pack(cuda, transposed):
  """Whole filter, a kernel input wider than the filter (mapped, with padding channels), and output-channel ranges at the
  front, in the middle and at the end of a filter of 544 rows — the two ranges of a 272 + 272 data gradient among them."""
  def both(w, cin_kernel, cmap, first, count):
    """(device pack of the range, host pack of the filter's slice)"""
    cm = None if cmap is None else torch.tensor(cmap, dtype=torch.int32, device='cuda')
    dev = ops.pack_wide_weights_dev(_dev(w), cin_kernel=cin_kernel, chan_map=cm, transposed=transposed, co_first=first, co_count=count)
    sl = w[:, :, first:first + count, :] if transposed else w[:, :, :, first:first + count]
    return dev.cpu().numpy(), ops.pack_wide_weights(np.ascontiguousarray(sl), cin_kernel=cin_kernel, chan_map=cmap, transposed=transposed)

  shape = lambda ci, co: (3, 3, co, ci) if transposed else (3, 3, ci, co)
  got, want = both(_filter(shape(20, 144), 1), None, None, 0, 144)
  assert np.array_equal(got, want)
  cmap = [0, 1, 2, -1] + list(range(3, 19)) + [-1, 19, -1, -1]  # 24 kernel channels, 20 filter rows
  got, want = both(_filter(shape(20, 272), 2), 24, cmap, 0, 272)
  assert np.array_equal(got, want)
  w = _filter(shape(16, 544), 3)
  for first, count in ((0, 272), (272, 272), (128, 144), (32, 512)):
    got, want = both(w, None, None, first, count)
    assert got.shape == want.shape and np.array_equal(got, want), (first, count)
  with pytest.raises(RecAttendError, match='channels'):
    ops.pack_wide_weights_dev(_dev(w), transposed=transposed, co_first=400, co_count=272)


# ------------------------------------------------------------------------- 2. one layer through the node against float64 autograd
# (name, transposed, stride, pool, c0, c1, cout) on a 2 x 6 x 10 map
LAYERS = [('144->144', False, 1, 1, 144, 0, 144), ('16->272 stride 2', True, 2, 1, 16, 0, 272), ('272+272->512', True, 1, 1, 272, 272, 512),
          ('512->16', False, 1, 1, 512, 0, 16), ('144->144 pool 2', False, 1, 2, 144, 0, 144), ('272+272->16', True, 1, 1, 272, 272, 16)]
LB, LH, LW = 2, 6, 10


@functools.lru_cache(maxsize=None)
def layer_reference(name):
  """Inputs (float32 host tensors) and the float64 autograd gradients of sum(y * dy) for one layer, through the oracle's own
  conv / transposed conv / BatchNorm restatements."""
  _, tr, stride, pool, c0, c1, cout = next(l for l in LAYERS if l[0] == name)
  rng = np.random.RandomState(len(name) + 7 * cout + c1)
  cin = c0 + c1
  f32 = lambda *s: torch.from_numpy(rng.randn(*s).astype(np.float32))
  x0, x1 = f32(LB, LH, LW, c0), (f32(LB, LH, LW, c1) if c1 else None)
  w = f32(*((3, 3, cout, cin) if tr else (3, 3, cin, cout))) * float(np.sqrt(2.0 / (9 * cin)))
  b, gamma, beta = 0.1 * f32(cout), 1.0 + 0.2 * f32(cout), 0.2 * f32(cout)
  dy = f32(LB, LH * stride // pool, LW * stride // pool, cout)
  leaves = [t.double().requires_grad_(True) if t is not None else None for t in (x0, x1, w, b, gamma, beta)]
  X0, X1, Wt, Bt, G, Be = leaves
  h = (X0 if X1 is None else torch.cat([X0, X1], dim=3)).permute(0, 3, 1, 2)
  if tr:
    u = fto._conv_transpose_same(h, Wt, stride) + Bt.view(1, -1, 1, 1)
  else:
    u = torch.nn.functional.conv2d(h, Wt.permute(3, 2, 0, 1), Bt, padding=1)
  y, mean, var = fto._bn_train(u, G, Be)
  y = torch.relu(y)
  if pool > 1:
    y = torch.nn.functional.max_pool2d(y, pool, pool)
  y = y.permute(0, 2, 3, 1)
  (y * dy.double()).sum().backward()
  grads = [None if t is None else t.grad for t in leaves]
  return (x0, x1, w, b, gamma, beta, dy), y.detach(), (mean.detach(), var.detach()), grads


def _rel(got, ref, floor=0.0):
  return float((got.detach().cpu().double() - ref).abs().max() / max(float(ref.abs().max()), floor))


@pytest.mark.parametrize('name', [l[0] for l in LAYERS])
def test_one_layer_through_the_node(cuda, name):
  """Bars: y 1e-4 of max (bn_form_cases' forward bar), moments 1e-5, dx and dW 2e-5 of max |ref| (the filter-gradient bar), dgamma
  / dbeta 1e-4 of max(1, max |ref|) (bn_form_cases' bars).  Once with fresh gradient tensors returned, once into a pre-filled
  bucket; twice for the bits."""
  _, tr, stride, pool, c0, c1, cout = next(l for l in LAYERS if l[0] == name)
  (x0, x1, w, b, gamma, beta, dy), yref, (mref, vref), gref = layer_reference(name)

  def run(bucket):
    lv = [None if t is None else t.cuda().requires_grad_(True) for t in (x0, x1, w, b, gamma, beta)]
    meta = dict(transposed=tr, stride=stride, pool=pool, relu=True, c0=c0, c1=c1, cache={})
    if bucket is not None:
      meta['grads'] = bucket
    y, mean, var = ra_fg_train.WideConvBNActPool.apply(*lv, meta)
    (y * dy.cuda()).sum().backward()
    return y, mean, var, lv

  y, mean, var, lv = run(None)
  errs = dict(y=_rel(y, yref), mean=_rel(mean, mref, 1.0), var=_rel(var, vref, 1.0), dx0=_rel(lv[0].grad, gref[0]), dw=_rel(lv[2].grad, gref[2]),
              dgamma=_rel(lv[4].grad, gref[4], 1.0), dbeta=_rel(lv[5].grad, gref[5], 1.0))
  if x1 is not None:
    errs['dx1'] = _rel(lv[1].grad, gref[1])
  print('node %-18s %s' % (name, '  '.join('%s %.2e' % kv for kv in errs.items())))
  bars = dict(y=1e-4, mean=1e-5, var=1e-5, dx0=2e-5, dx1=2e-5, dw=2e-5, dgamma=1e-4, dbeta=1e-4)
  assert all(v <= bars[k] for k, v in errs.items()), errs
  # the bias feeds BatchNorm: its true gradient is zero (the whole graph's bar: 2e-3 of the gradients' scale)
  assert float(lv[3].grad.abs().max()) <= 2e-3 * float(gref[2].abs().max())
  # into a bucket that already holds values: added, one writer per element, and nothing is returned for the parameters
  fill = [torch.full_like(t, v).cuda() for t, v in ((w, 0.5), (b, -1.0), (gamma, 2.0), (beta, 3.0))]
  y2, _, _, lv2 = run(tuple(fill))
  assert torch.equal(y, y2) and all(lv2[k].grad is None for k in (2, 3, 4, 5))
  for got, plain, v in zip(fill, (lv[2].grad, lv[3].grad, lv[4].grad, lv[5].grad), (0.5, -1.0, 2.0, 3.0)):
    assert torch.equal(got, plain + v)
  assert torch.equal(lv2[0].grad, lv[0].grad) and (x1 is None or torch.equal(lv2[1].grad, lv[1].grad))  # no atomics anywhere


# --------------------------------------------------------------------------------- 3. the whole graph against float64 autograd
B, H, W = 2, 16, 24
WIDE_NETS = [(1, 'bce'), (3, 'iou'), (9, 'bce')]


def wide_opt(nsc, seg, **kw):
  """Wide layers on both sides of the bottleneck: cnn 1 (8 -> 144), cnn 2 (144 -> 272), dcnn 0 (32 -> 272, stride 2), dcnn 1
  (272 + 272 -> 512: two data-gradient ranges, BatchNorm at 512); narrow layers behind wide inputs: cnn 3 (272 -> 32), dcnn 2
  (512 -> 16, stride 2); dcnn 3 reads its 16 channels + the image."""
  return dict(inp_depth=3, cnn_filter_size=[3] * 4, cnn_depth=[8, 144, 272, 32], cnn_pool=[1, 2, 1, 2], cnn_skip_mask=[True, False, False, True],
              dcnn_filter_size=[3] * 5, dcnn_depth=[272, 512, 16, 12, nsc + 8], dcnn_pool=[2, 1, 2, 1, 1],
              dcnn_skip_mask=[True, False, True, False], use_bn=True, add_skip_conn=True, add_orientation=True, num_orientation_classes=8,
              num_semantic_classes=nsc, weight_decay=5e-5, padding=2, segm_loss_fn=seg, rnd_hflip=False, rnd_vflip=False, rnd_transpose=False,
              rnd_colour=False, base_learn_rate=1e-3, learn_rate_decay=0.96, steps_per_learn_rate_decay=5000, optimizer='adam', **kw)


@functools.lru_cache(maxsize=None)
def wide_reference(nsc, seg):
  opt = wide_opt(nsc, seg)
  assert fg_model.derive(opt)['dcnn_in_ch'] == [32, 544, 512, 19, 12]
  P = fo.random_weights(opt, 11 + nsc)
  x, y, d = graph_batch(nsc, True, 21 + nsc)
  return opt, P, (x, y, d), fto.train_graph(opt, P, x, y, d, draws=DRAWS)


@pytest.mark.parametrize('nsc,seg', WIDE_NETS)
def test_wide_whole_graph_vs_float64_autograd(cuda, nsc, seg):
  """The bars of test_fg_train_gpu.test_whole_graph_vs_float64_autograd: pieces 2e-4, moments and shadows 1e-5, per tensor 5 %,
  cosine 0.9995, pre-BN biases 2e-3 of the scale."""
  opt, P, (x, y, d), ref = wide_reference(nsc, seg)
  model = fg_model.get_model(opt).load_weights(P)
  names = fg_model.save_var_names(model)
  with pytest.raises(RecAttendError, match='is not built'):
    ra_fg_train.FgTrainStep(model)
  ts = ra_fg_train.FgTrainStep(model, wide=True)
  ts.bucket.zero_grad()
  loss, pieces, stats = ts.forward_loss(_dev(x), _dev(y), _dev(d), draws=DRAWS)
  loss.backward()
  assert np.array_equal(pieces['x_trans'].cpu().numpy(), ref['x_trans'].astype(np.float32))
  assert set(ref['pieces']) == set(k for k in ra_fg_train.FETCHES if k in pieces)
  for k, v in ref['pieces'].items():
    print('%-16s %.8g (oracle %.8g)' % (k, float(pieces[k]), v))
    assert abs(float(pieces[k]) - v) < 2e-4 * max(1.0, abs(v)), k
  assert abs(float(loss.detach()) - ref['pieces']['loss']) < 2e-4 * max(1.0, abs(ref['pieces']['loss']))
  assert set(stats) == set(names[pre + '/bn/gamma'][:-len('_gamma')] for pre in ref['moments'])
  worst_m = 0.0
  for pre, (mean, var) in ref['moments'].items():
    key = names[pre + '/bn/gamma'][:-len('_gamma')]
    for got, want, what in ((stats[key][0], mean, 'mean'), (stats[key][1], var, 'var'),
                            (model[key + '_ema_mean'], ref['ema'][pre + '/bn/ema_mean'], 'ema_mean'),
                            (model[key + '_ema_var'], ref['ema'][pre + '/bn/ema_var'], 'ema_var')):
      e = np.abs(got.cpu().numpy() - want).max() / max(1.0, np.abs(want).max())
      worst_m = max(worst_m, e)
      assert e < 1e-5, (pre, what, e)
  cos, worst = compare_grads(ref['data_grads'], lambda k: ts.bucket.grad_of[names[k]].cpu().numpy().astype(np.float64), opt)
  print('moments %.2e, gradient cosine %.8f, worst per-tensor relative error %.2e (%s)' % (worst_m, cos, max(worst.values()), max(worst, key=worst.get)))
  bad = {k: v for k, v in worst.items() if v > 5e-2}
  assert cos >= 0.9995 and not bad, (cos, sorted(bad.items(), key=lambda kv: -kv[1])[:8])


# --------------------------------------------------------------------------------------------------------- 4. the real nets
def _batch(nsc, n, h, w, seed, fg=0.4):
  rng = np.random.RandomState(seed)
  x = rng.rand(n, h, w, 3).astype(np.float32)
  if nsc == 1:
    y = (rng.rand(n, h, w) < fg).astype(np.float32)
  else:
    y = np.eye(nsc, dtype=np.float32)[np.where(rng.rand(n, h, w) < fg, rng.randint(1, nsc, (n, h, w)), 0)]
  return x, y, np.eye(8, dtype=np.float32)[rng.randint(0, 8, (n, h, w))]


@pytest.mark.parametrize('net,h,w', [('kitti', 64, 128), ('cityscapes', 64, 64)])
def test_run_script_nets_take_a_pass(cuda, net, h, w):
  """One forward_loss + backward of the nets run_kitti.sh / run_cityscapes.sh train, B = 2: the loss pieces against the float64
  oracle at 2e-4, every bucket gradient finite.  Moments and gradients are NOT compared: at these map sizes the deepest BatchNorm
  sees 16 or 8 samples per channel, and float32 torch alone is off by 8.5e-6 / 2.0e-5 in the moments and by 3.8 % / 8.7 % in the
  worst tensor; the kernels would be blamed for the conditioning."""
  opt = fo.kitti_opt() if net == 'kitti' else fo.cityscapes_opt()
  nsc = opt['num_semantic_classes']
  P = fo.random_weights(opt, 5)
  x, y, d = _batch(nsc, 2, h, w, 6)
  ref = fto.train_graph(opt, P, x, y, d, draws=DRAWS)
  model = fg_model.get_model(opt).load_weights(P)
  ts = ra_fg_train.FgTrainStep(model, wide=True)
  ts.bucket.zero_grad()
  loss, pieces, _ = ts.forward_loss(_dev(x), _dev(y), _dev(d), draws=DRAWS)
  loss.backward()
  for k, v in ref['pieces'].items():
    print('%s %-16s %.8g (oracle %.8g)' % (net, k, float(pieces[k]), v))
    assert abs(float(pieces[k]) - v) < 2e-4 * max(1.0, abs(v)), k
  assert bool(torch.isfinite(ts.bucket.grad).all()) and float(ts.bucket.grad.abs().max()) > 0


# ------------------------------------------------------------------------------------------------------- 5. trainer behaviour
def _small_trainer(optimizer='adam', lr=1e-3, seed=31, **kw):
  opt = wide_opt(3, 'bce', **kw)
  opt.update(optimizer=optimizer, base_learn_rate=lr)
  model = fg_model.get_model(opt).load_weights(fo.random_weights(opt, seed))
  return model, ra_fg_train.FgTrainStep(model, wide=True)


@pytest.mark.parametrize('optimizer,lr', [('adam', 1e-3), ('momentum', 1e-2)])
def test_wide_five_steps_on_one_batch(cuda, optimizer, lr):
  model, ts = _small_trainer(optimizer, lr)
  shadows = {k: model[k].clone() for k in model if isinstance(k, str) and k.endswith(('_ema_mean', '_ema_var'))}
  x, y, d = (_dev(a) for a in graph_batch(3, True, 32))
  losses = [float(ts.run(x, y, d, draws=DRAWS)['loss']) for _ in range(5)]
  ts.flush_status()
  print('%s: losses %s' % (optimizer, ' '.join('%.5f' % v for v in losses)))
  assert np.isfinite(losses).all() and losses[-1] < losses[0]
  assert shadows and all(not torch.equal(v, model[k]) for k, v in shadows.items())
  before = model.statistics(x, y, d)
  ts.sync_model()
  after = model.statistics(x, y, d)  # the eval closures (K1-wide at eval) see the trained weights
  assert np.isfinite(after['loss']) and after['loss'] != before['loss']


def test_wide_step_without_foreground_is_skipped(cuda):
  model, ts = _small_trainer('momentum', 1e-2, seed=5)
  x, y, d = graph_batch(3, True, 6)
  ts.run(_dev(x), _dev(y), _dev(d))
  ts.flush_status()
  keep = [t.clone() for t in (ts.bucket.param, ts.accum, ts.bucket.m, ts.bucket.v)]
  y0 = np.zeros_like(y)
  y0[..., 0] = 1
  out = ts.run(_dev(x), _dev(y0), _dev(d))
  assert np.isnan(float(out['loss']))
  for a, t in zip(keep, (ts.bucket.param, ts.accum, ts.bucket.m, ts.bucket.v)):
    assert torch.equal(a, t)
  with pytest.raises(RecAttendError, match='no foreground pixel'):
    ts.flush_status()
  assert ts.bucket.global_step == 1


def test_wide_backward_is_bit_reproducible(cuda):
  model, ts = _small_trainer(seed=5)
  x, y, d = (_dev(a) for a in graph_batch(3, True, 6))
  buckets = []
  for _ in range(2):
    ts.bucket.zero_grad()
    loss, _, _ = ts.forward_loss(x, y, d, draws=DRAWS)
    loss.backward()
    buckets.append(ts.bucket.grad.clone())
  assert torch.equal(buckets[0], buckets[1]) and float(buckets[0].abs().max()) > 0


def test_wide_train_eval_restore_chain(cuda, tmp_path, capsys):
  """fg_model_train.py --train_wide ... --save_ckpt -> fg_model_eval.py --model_id -> --restore, as
  test_fg_train_gpu.test_train_pack_eval_chain does for a narrow net."""
  rng = np.random.RandomState(41)
  n = 4
  x, y, d = graph_batch(1, True, 42, n=n)
  src = str(tmp_path / 'train.npz')
  np.savez(src, x=x, y_gt=y, d_gt=d, fg_gt_full=(rng.rand(n, 2 * H, 2 * W) < 0.4).astype(np.uint8))
  res = str(tmp_path / 'results')
  net = ('--cnn_depth 8,144,272,32 --cnn_pool 1,2,1,2 --cnn_skip_mask 1,0,0,1 --dcnn_depth 272,512,16,12,9 --dcnn_pool 2,1,2,1,1 '
         '--dcnn_skip_mask 1,0,1,0 --add_skip_conn --add_orientation --segm_loss_fn bce --optimizer momentum --padding 2').split()
  common = net + ['--model_id', 'fgw', '--results', res, '--input', src, '--batch_size', '2', '--steps_per_log', '1']
  with pytest.raises(RecAttendError, match='--train_wide'):  # the default refuses the net and names the flag
    fg_model_train.main(common + ['--num_steps', '1'])
  tr = fg_model_train.main(common + ['--train_wide', '--num_steps', '3', '--save_ckpt', '--steps_per_ckpt', '2'])
  assert tr.wide and tr.bucket.global_step == 3
  folder = os.path.join(res, 'fgw')
  import yaml
  with open(os.path.join(folder, 'model_opt.yaml')) as f:
    opt = yaml.safe_load(f)
  assert opt['train_wide'] is True
  weights = dict(np.load(os.path.join(folder, 'weights.npz')))
  model = fg_model.get_model(opt).load_weights(weights)  # strict
  for k, v in tr.model.state_dict_numpy().items():
    assert np.array_equal(weights[k], v), k
  out = fg_model_eval.main(['--model_id', 'fgw', '--results', res, '--input', src, '--output', str(tmp_path / 'eval'), '--batch_size', '2'])
  assert all(np.isfinite(v) for v in out['statistics'].values())
  state = dict(np.load(os.path.join(folder, 'optimizer.npz')))
  capsys.readouterr()
  tr2 = fg_model_train.main(['--model_id', 'fgw2', '--results', res, '--input', src, '--batch_size', '2', '--restore', folder,
                             '--num_steps', '4', '--steps_per_log', '1'])  # no --train_wide: the restored run's options carry it
  text = capsys.readouterr().out
  assert tr2.wide and 'restored' in text and 'global_step 3' in text and '\nstep 3 ' in text and '\nstep 2 ' not in text
  assert tr2.bucket.global_step == 4 and int(state['global_step']) == 3
