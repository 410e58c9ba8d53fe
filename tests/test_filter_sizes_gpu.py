"""Filter sizes 1, 5 and 7 in the cnn / dcnn layers on the MI355X (ra_convkxk_f32, nnlib.py:131-257, :260-404), against
the float64 NumPy oracle: the kernel layer by layer (SAME conv + bias + BN + ReLU + 2x2 max-pool; SAME conv2d_transpose
stride 1 and 2 over concat(prev, skip); the canvas plane), then full_model / box_model end to end with mixed sizes,
the captured-graph pipeline, and the refusal to train."""
import numpy as np
import pytest
import torch

import ra_ops as ops
import ra_oracle as ora
from ra_native import RecAttendError

pytestmark = pytest.mark.gpu
MASK_TOL = 1e-3  # tests/test_full_model_gpu.py's bars


def _dev(a):
  return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def _layer(kf, H, c0, c1, cout, pool, mode, plane, seed, B=2):
  """One layer through ops.conv2d_fused and the oracle.  mode: 'conv' | 'tconv1' | 'tconv2' (conv2d_transpose, stride)."""
  rng = np.random.RandomState(seed)
  x0 = rng.randn(B, H, H, c0).astype(np.float32)
  x1 = rng.randn(B, H, H, c1).astype(np.float32) if c1 else None
  cin = c0 + c1
  tr = mode != 'conv'
  w = (rng.randn(kf, kf, cout, cin) if tr else rng.randn(kf, kf, cin, cout)).astype(np.float32) / np.sqrt(kf * kf * cin)
  b = rng.normal(0, 0.1, cout).astype(np.float32)
  bn = (rng.normal(0.1, 0.2, cout), rng.uniform(0.7, 1.4, cout), rng.normal(0, 0.2, cout), rng.uniform(0.5, 1.5, cout))
  bn = tuple(a.astype(np.float32) for a in bn)
  pl, pc = None, -1
  xin = x0 if x1 is None else np.concatenate([x0, x1], axis=3)
  if plane:  # the canvas in its own plane stands in for channel 3 of the packed input
    pl, pc = rng.rand(B, H, H).astype(np.float32), 3
    xin = xin.copy()
    xin[..., pc] = pl
  sc, sh = ops.fold_bn(b, cout, bn)
  wp = ops.pack_conv_weights(w, transposed=tr)
  y = ops.conv2d_fused(_dev(x0), _dev(wp), _dev(sc), _dev(sh), cout, kf, relu=True, pool=pool,
                       src1=None if x1 is None else _dev(x1), upsample=(mode == 'tconv2'),
                       plane=None if pl is None else _dev(pl), plane_chan=pc)
  torch.cuda.synchronize()
  x64, w64 = xin.astype(np.float64), w.astype(np.float64)
  if mode == 'conv':
    a = ora.conv2d(x64, w64)
  else:
    a = ora.conv2d_transpose(x64, w64, 2 if mode == 'tconv2' else 1)
  a = ora.relu(ora.batch_norm_eval(a + b, *[v.astype(np.float64) for v in bn]))
  ref = ora.max_pool(a, pool) if pool > 1 else a
  return y.cpu().numpy(), ref


# (H, C0, C1, Cout) from the run scripts' layers: the packed model input (4 = CVPPP, 16 = KITTI's 13 packed) with the canvas
# plane, the controller CNN at 128, the attention CNN on the 48 x 48 patch down to 6 x 6
CONV = [(128, 4, 0, 8, True), (128, 8, 0, 16, False), (128, 16, 0, 16, True), (48, 16, 0, 32, False),
        (48, 32, 0, 64, False), (12, 64, 0, 96, False), (6, 96, 0, 64, False)]
# the attention DCNN: stride 1 and 2 over concat(prev, skip), down to the 1-channel mask
TCONV = [(12, 96, 0, 64, 'tconv2'), (6, 64, 64, 32, 'tconv2'), (24, 16, 16, 16, 'tconv2'), (24, 32, 32, 32, 'tconv1'),
         (48, 8, 4, 1, 'tconv1'), (48, 16, 0, 8, 'tconv1')]


@pytest.mark.parametrize('kf', [1, 5, 7])
@pytest.mark.parametrize('pool', [1, 2])
@pytest.mark.parametrize('H,c0,c1,cout,plane', CONV)
def test_kernel_conv_vs_oracle(cuda, kf, pool, H, c0, c1, cout, plane):
  y, ref = _layer(kf, H, c0, c1, cout, pool, 'conv', plane, seed=kf * 1000 + H + c0 + cout + pool)
  assert y.shape == ref.shape
  err = np.abs(y - ref).max()
  assert err <= 1e-4 * np.abs(ref).max(), (err, np.abs(ref).max())


@pytest.mark.parametrize('kf', [1, 5, 7])
@pytest.mark.parametrize('H,c0,c1,cout,mode', TCONV)
def test_kernel_transposed_vs_oracle(cuda, kf, H, c0, c1, cout, mode):
  y, ref = _layer(kf, H, c0, c1, cout, 1, mode, False, seed=kf * 1000 + H + c0 + c1 + cout)
  assert y.shape == ref.shape
  err = np.abs(y - ref).max()
  assert err <= 1e-4 * np.abs(ref).max(), (err, np.abs(ref).max())


def test_kernel_three_by_three_is_conv3x3(cuda):
  """ksize = 3 through conv2d_fused / ra_convkxk_f32 IS ra_conv3x3_f32: the same bits."""
  rng = np.random.RandomState(3)
  x = _dev(rng.randn(2, 48, 48, 16))
  w = rng.randn(3, 3, 16, 32).astype(np.float32) / 12
  wp, (sc, sh) = _dev(ops.pack_conv_weights(w)), ops.fold_bn(rng.randn(32).astype(np.float32), 32)
  a = ops.conv3x3(x, wp, _dev(sc), _dev(sh), 32, pool=2)
  b = ops.conv2d_fused(x, wp, _dev(sc), _dev(sh), 32, 3, pool=2)
  assert torch.equal(a, b)


def _redraw_filters(P, opt, seed, box_model=False):
  """ora.random_params draws 3x3 filters: redraw every conv filter at its configured size (fan-in f^2 * cin)."""
  rng = np.random.RandomState(seed)
  P = dict(P)
  nets = [('ctrl_cnn', opt['ctrl_cnn_filter_size'], False)]
  if not box_model:
    nets += [('attn_cnn', opt['attn_cnn_filter_size'], False), ('attn_dcnn', opt['attn_dcnn_filter_size'], True)]
  for scope, fs, tr in nets:
    for i, f in enumerate(fs):
      k = '%s_w_%d' % (scope, i)
      shp = (f, f) + P[k].shape[2:]
      cin = shp[3] if tr else shp[2]
      P[k] = rng.normal(0.0, 1.3 / np.sqrt(f * f * cin), shp).astype(np.float32)
  return P


def _inputs(opt, B, seed):
  rng = np.random.RandomState(seed)
  H, W = opt['inp_height'], opt['inp_width']
  x = rng.rand(B, H, W, 3).astype(np.float32)
  d_in = y_in = None
  if opt.get('add_d_out'):
    d_in = np.eye(8, dtype=np.float32)[rng.randint(0, 8, (B, H, W))]
    y_in = ora.softmax(rng.randn(B, H, W, opt['num_semantic_classes'])).astype(np.float32)
  return x, d_in, y_in


NAMES = ['y_out', 's_out', 'x_patch', 'y_out_patch', 'attn_ctr', 'attn_size', 'ctrl_rnn_glimpse_map', 'ctrl_out',
         'attn_box', 'canvas']


def _compare(out, ref):
  for k in NAMES:  # (the canvas comes back [B, H, W], the oracle's is [B, H, W, 1])
    assert out[k].size == ref[k].size, k
    out[k] = out[k].reshape(ref[k].shape)
  assert np.abs(out['attn_ctr'] - ref['attn_ctr']).max() < 2e-3
  assert np.abs(out['attn_size'] - ref['attn_size']).max() < 2e-3
  assert np.abs(out['ctrl_out'] - ref['ctrl_out']).max() < 2e-3
  assert np.abs(out['ctrl_rnn_glimpse_map'] - ref['ctrl_rnn_glimpse_map']).max() < 1e-4
  assert np.abs(out['x_patch'] - ref['x_patch']).max() < 1e-3
  assert np.abs(out['y_out_patch'] - ref['y_out_patch']).max() < 1e-3
  for k in ('y_out', 's_out', 'attn_box', 'canvas'):
    assert np.abs(out[k] - ref[k]).max() < MASK_TOL, k


def _full_case(opt, B, seed):
  import full_model
  P = _redraw_filters(ora.random_params(opt, seed), opt, seed + 7)
  x, d_in, y_in = _inputs(opt, B, seed + 1)
  ref = ora.full_model_forward(opt, P, x, d_in, y_in)
  m = full_model.get_model(opt).load_weights(P)
  feed = {'x': x, 'phase_train': False, 'd_in': d_in, 'y_in': y_in}
  return m, feed, ref


def test_full_model_cvppp_mixed_sizes_vs_oracle(cuda):
  opt = ora.make_opt('cvppp', 128, 128, 3, ctrl_cnn_filter_size=[5, 3, 1, 3, 7, 3, 3, 3],
                     attn_cnn_filter_size=[5, 3, 1, 3, 7, 3], attn_dcnn_filter_size=[3, 5, 5, 7, 1, 3, 1])
  m, feed, ref = _full_case(opt, 2, 61)
  for rep in range(2):  # the second pass replays the captured graph
    out = dict(zip(NAMES, m.run(NAMES, feed, as_numpy=True)))
    _compare(out, ref)


def test_full_model_kitti_mixed_sizes_vs_oracle(cuda):
  """64 x 96 with d_in / y_in, skip connections, stride-2 DCNN layers of sizes 7, 5 and 3."""
  opt = ora.make_opt('kitti', 64, 96, 2, ctrl_cnn_filter_size=[3, 5, 3, 1, 3, 7, 3, 3],
                     attn_cnn_filter_size=[1, 3, 5, 3, 7, 3], attn_dcnn_filter_size=[7, 3, 5, 1, 3, 5, 1])
  m, feed, ref = _full_case(opt, 2, 62)
  out = dict(zip(NAMES, m.run(NAMES, feed, as_numpy=True)))
  _compare(out, ref)


def test_box_model_mixed_sizes_vs_oracle(cuda):
  import box_model
  T, B, H, W = 3, 2, 96, 96
  opt = ora.make_opt('cvppp', H, W, T, ctrl_cnn_filter_size=[7, 3, 5, 1, 3, 5, 3, 1])
  P = _redraw_filters(ora.random_params(opt, 9, box_model=True), opt, 10, box_model=True)
  rng = np.random.RandomState(11)
  x = rng.rand(B, H, W, 3).astype(np.float32)
  y_gt = np.zeros((B, T, H, W), np.float32)
  y_gt[:, 0, 10:40, 15:50] = 1
  y_gt[:, 1, 50:80, 40:90] = 1
  noise = rng.uniform(0, 0.3, (T, B, H, W, 1)).astype(np.float32)
  ref = ora.box_model_forward(opt, P, x, y_gt, noise)
  m = box_model.get_model(opt).load_weights(P)
  names = ['s_out', 'attn_box', 'attn_ctr', 'attn_size', 'canvas']
  for rep in range(2):
    out = dict(zip(names, m.run(names, {'x': x, 'y_gt': y_gt, 'noise': noise[..., 0], 'phase_train': False},
                                as_numpy=True)))
    for k in names:
      assert np.abs(out[k] - ref[k]).max() < (2e-3 if k.startswith('attn_c') or k == 'attn_size' else MASK_TOL), k


def test_pipeline_coalesced_mixed_sizes(cuda):
  """The timed path: DecodePipeline(2, coalesce=2) on captured graphs returns what lone runs return, and the oracle's masks."""
  opt = ora.make_opt('cvppp', 128, 128, 2, ctrl_cnn_filter_size=[3, 5, 3, 1, 3, 3, 7, 3],
                     attn_cnn_filter_size=[3, 3, 5, 3, 3, 1], attn_dcnn_filter_size=[5, 3, 3, 7, 3, 3, 1])
  m, feed, ref = _full_case(opt, 2, 63)
  rng = np.random.RandomState(64)
  feeds = [feed] + [{'x': rng.rand(2, 128, 128, 3).astype(np.float32), 'phase_train': False} for _ in range(3)]
  names = ['y_out', 's_out', 'x_patch']
  lone = [m.run(names, f, as_numpy=True) for f in feeds]
  pipe = m.pipeline(2, coalesce=2)
  got = []
  for f in feeds:
    while pipe.full(f['x'].shape[0]):
      got.append(pipe.collect(as_numpy=True))
    pipe.submit(names, f)
  while len(pipe):
    got.append(pipe.collect(as_numpy=True))
  assert len(got) == len(lone)
  for a, b in zip(got, lone):
    for u, v in zip(a, b):
      assert u.shape == v.shape and np.abs(u - v).max() < 1e-6
  assert np.abs(got[0][0] - ref['y_out']).max() < MASK_TOL and np.abs(got[0][1] - ref['s_out']).max() < MASK_TOL


def test_training_refused_for_other_sizes(cuda):
  import full_model
  opt = ora.make_opt('cvppp', 64, 64, 2, attn_cnn_filter_size=[3, 5, 3, 3, 3, 3])
  m = full_model.get_model(opt).load_weights(_redraw_filters(ora.random_params(opt, 5), opt, 6))
  rng = np.random.RandomState(7)
  feed = {'x': rng.rand(2, 64, 64, 3).astype(np.float32), 'y_gt': np.zeros((2, 2, 64, 64), np.float32),
          's_gt': np.zeros((2, 2), np.float32), 'phase_train': True}
  with pytest.raises(RecAttendError, match='3x3'):
    m.run(['loss', 'train_step'], feed)


def test_eval_cli_decodes_a_mixed_size_checkpoint(cuda, tmp_path):
  """results/<id>/{model_opt.yaml, weights.npz} with 1 / 3 / 5 / 7 filters loads and decodes through full_model_eval.py."""
  import yaml
  import full_model
  import full_model_eval
  opt = ora.make_opt('cvppp', 64, 64, 3, ctrl_cnn_filter_size=[1, 5, 3, 7, 3, 3, 5, 3],
                     attn_cnn_filter_size=[7, 3, 5, 1, 3, 3], attn_dcnn_filter_size=[5, 1, 7, 3, 5, 3, 7])
  P = _redraw_filters(ora.random_params(opt, 21), opt, 22)
  folder = tmp_path / 'results' / 'mix'
  folder.mkdir(parents=True)
  with open(str(folder / 'model_opt.yaml'), 'w') as f:
    yaml.safe_dump(opt, f)
  np.savez(str(folder / 'weights.npz'), **P)
  x = np.random.RandomState(23).rand(3, 64, 64, 3).astype(np.float32)
  inp = str(tmp_path / 'in.npz')
  np.savez(inp, x=x)
  full_model_eval.main(['--model_id', 'mix', '--results', str(tmp_path / 'results'), '--input', inp, '--batch_size', '2'])
  pred = np.load(str(folder / 'output_valid' / 'pred_rank0.npz'))
  assert pred['y_out'].shape == (3, 3, 64, 64) and pred['s_out'].shape == (3, 3)
  ref = ora.full_model_forward(opt, P, x)
  assert np.abs(pred['s_out'] - ref['s_out']).max() < MASK_TOL
  m = full_model.get_model(opt).load_weights(P)
  y, s = m.run(['y_out', 's_out'], {'x': x, 'phase_train': False}, as_numpy=True)
  assert np.abs(y - ref['y_out']).max() < MASK_TOL and np.abs(s - pred['s_out']).max() < 1e-6
