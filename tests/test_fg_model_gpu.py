"""fg_model at eval on the MI355X: the wide 3x3 layer (ra_conv3x3_wide_f32) and the head (ra_fg_head_f32) against the
float64 oracle, the nets of run_kitti.sh / run_cityscapes.sh end to end, the 8-bit round trip, the chained run into the
decode engine and the two command lines.  Bars: 2e-5 relative to the largest reference value for the kernel (the 3x3 K1's bar
in test_kernels_gpu.py) and 2e-5 on y_out / d_out (the project's mask tolerance); float32 torch on a CPU sits at
3e-7 .. 5e-7 on the same nets."""
import functools
import os

import numpy as np
import pytest
import torch

import fg_model
import fg_oracle as fo
import ra_native as rn
import ra_ops as ops
import ra_oracle as ora

pytestmark = pytest.mark.gpu
TOL = 2e-5


def _dev(a):
  return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


# ---- 7. / 8. the wide kernel
SHAPES = [(8, 28, 256, 0, 512), (4, 14, 512, 0, 256), (8, 28, 256, 256, 256), (8, 16, 512, 512, 512), (4, 8, 512, 0, 512),
          (16, 56, 128, 0, 256), (32, 64, 192, 192, 192), (64, 128, 128, 0, 192), (6, 10, 132, 4, 144)]
MODES = ['conv1', 'conv2', 'tconv1', 'tconv2']  # conv with pool 1 / 2; conv2d_transpose stride 1 / 2 (dcnn never pools)


@functools.lru_cache(maxsize=2)
def _wide_case(shape, mode):
  """Inputs of a layer at B = 3 and its float64 pre-activation (conv + bias -> BN); B = 1 is the first image."""
  H, W, c0, c1, cout = shape
  rng = np.random.RandomState(sum(shape) * 4 + MODES.index(mode))
  B, cin, tr = 3, c0 + c1, mode.startswith('t')
  x0 = rng.randn(B, H, W, c0).astype(np.float32)
  x1 = rng.randn(B, H, W, c1).astype(np.float32) if c1 else None
  w = (rng.randn(3, 3, cout, cin) if tr else rng.randn(3, 3, cin, cout)).astype(np.float32) / np.sqrt(9 * cin)
  b = rng.normal(0, 0.1, cout).astype(np.float32)
  bn = tuple(a.astype(np.float32) for a in (rng.normal(0.1, 0.2, cout), rng.uniform(0.7, 1.4, cout), rng.normal(0, 0.2, cout),
                                            rng.uniform(0.5, 1.5, cout)))
  xin = (x0 if x1 is None else np.concatenate([x0, x1], axis=3)).astype(np.float64)
  w8 = w.astype(np.float64)
  u = ora.conv2d_transpose(xin, w8, 2 if mode == 'tconv2' else 1) if tr else ora.conv2d(xin, w8)
  u = ora.batch_norm_eval(u + b.astype(np.float64), *[a.astype(np.float64) for a in bn])
  sc, sh = ops.fold_bn(b, cout, bn)
  wp = ops.pack_conv_weights(w, transposed=tr)
  return x0, x1, u, _dev(wp), _dev(sc), _dev(sh)


def _run_wide(case, shape, mode, relu, B):
  x0, x1, _, wp, sc, sh = case
  return ops.conv2d_fused(_dev(x0[:B]), wp, sc, sh, shape[4], 3, relu=relu, pool=2 if mode == 'conv2' else 1,
                          src1=None if x1 is None else _dev(x1[:B]), upsample=mode == 'tconv2')


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(str(v) for v in s))
def test_wide_layer_matches_float64_oracle(cuda, shape, mode):
  case = _wide_case(shape, mode)
  for relu in (True, False):
    ref = ora.relu(case[2]) if relu else case[2]
    if mode == 'conv2':
      ref = ora.max_pool(ref, 2)
    for B in (1, 3):
      y = _run_wide(case, shape, mode, relu, B).cpu().numpy()
      r = ref[:B]
      assert y.shape == r.shape
      err = np.abs(y - r).max() / np.abs(r).max()
      print('wide %s %s relu=%d B=%d: max|y - ref| / max|ref| = %.3g' % (shape, mode, relu, B, err))
      assert err < TOL, (shape, mode, relu, B, err)


@pytest.mark.parametrize('shape,mode', [((8, 16, 512, 512, 512), 'conv2'), ((4, 8, 512, 0, 512), 'tconv2'),
                                        ((6, 10, 132, 4, 144), 'tconv1')])
def test_wide_layer_is_run_to_run_identical(cuda, shape, mode):
  case = _wide_case(shape, mode)
  a = _run_wide(case, shape, mode, True, 3)
  b = _run_wide(case, shape, mode, True, 3)
  assert torch.equal(a, b)


def test_wide_layer_refuses_other_shapes(cuda):
  x = torch.zeros(1, 8, 8, 64, device='cuda')
  one = torch.ones(520, device='cuda')
  with pytest.raises(rn.RecAttendError):
    ops.conv_wide(x, one, one, one, 520)
  with pytest.raises(rn.RecAttendError, match='3x3'):
    ops.conv2d_fused(x, one, one, one, 256, 5)


# ---- 9. the head
@pytest.mark.parametrize('nsc,no', [(1, 8), (9, 8), (1, 0), (3, 0)])
def test_head(cuda, nsc, no):
  rng = np.random.RandomState(nsc * 10 + no)
  B, H, W, D, Cp = 2, 12, 20, 3, 4 * (-(-(3 + 1 + no + nsc) // 4))
  lg = (rng.randn(B, H, W, nsc + no) * 2.5).astype(np.float32)
  l8 = lg.astype(np.float64)
  y_ref = ora.sigmoid(l8[..., :nsc]) if nsc == 1 else ora.softmax(l8[..., :nsc])
  d_ref = ora.softmax(l8[..., nsc:]) if no else None
  y, d = ops.fg_head(_dev(lg), nsc, no)
  assert np.abs(y.cpu().numpy() - y_ref).max() < 1e-6
  assert (d is None) == (no == 0)
  if no:
    assert np.abs(d.cpu().numpy() - d_ref).max() < 1e-6
  yq, dq = ops.fg_head(_dev(lg), nsc, no, quantise=True)
  _check_quantised(yq.cpu().numpy(), y_ref)
  if no:
    _check_quantised(dq.cpu().numpy(), d_ref)
  if no:  # the packed destination = ra_pack_input_plane_f32 fed with the head's own y_in / d_in, bit for bit
    x = _dev(rng.rand(B, H, W, D))
    packed = torch.full((B, H, W, Cp), 7.0, device='cuda')
    plane = torch.full((B, H, W), 7.0, device='cuda')
    y2, d2 = ops.fg_head(_dev(lg), nsc, no, quantise=True, x=x, packed=packed, canvas_plane=plane)
    assert torch.equal(y2, yq) and torch.equal(d2, dq)
    want, wplane = torch.full_like(packed, 5.0), torch.full_like(plane, 5.0)
    ops.pack_input(x, dq, yq, Cp, want, canvas_plane=wplane)
    assert torch.equal(packed, want) and torch.equal(plane, wplane)


def _check_quantised(got, ref64):
  """Item 11's rule: never more than one step from the oracle's 8-bit value, and equal wherever the oracle's v * 255 is farther
  than 2e-5 * 255 from an integer; the values that clause leaves out are at most 3 % of all."""
  want = fo.quantise(ref64)
  assert got.dtype == np.float32 and got.shape == want.shape
  k = got * np.float32(255)
  assert (k == np.round(k)).all() and got.min() >= 0 and got.max() <= 1
  steps = np.abs(np.round(k) - np.round(want * np.float32(255)))
  assert steps.max() <= 1
  v = ref64 * 255
  clear = np.abs(v - np.round(v)) > TOL * 255
  print('quantised: %.3f %% of the values within 2e-5 * 255 of an integer, %d of %d differ by one step' %
        (100 * (1 - clear.mean()), int(steps.sum()), steps.size))
  assert 1 - clear.mean() <= 0.03
  assert (steps[clear] == 0).all()


# ---- 10. / 11. end to end
NETS = {'kitti': (fo.kitti_opt, (2, 128, 448, 3), 21), 'cityscapes': (fo.cityscapes_opt, (1, 128, 256, 3), 22),
        'reduced': (lambda: fo.reduced_opt(nsc=3, orientation=False, wide=True), (2, 32, 48, 3), 23)}


@functools.lru_cache(maxsize=3)
def _net(name):
  make, shape, seed = NETS[name]
  opt = make()
  P = fo.random_weights(opt, seed)
  x = np.random.RandomState(seed + 100).rand(*shape).astype(np.float32)
  return opt, P, x, fo.forward(opt, P, x)


@pytest.mark.parametrize('name', sorted(NETS))
def test_end_to_end_matches_float64_oracle(cuda, name):
  opt, P, x, ref = _net(name)
  assert np.ptp(ref['y_out']) > 0.2  # saturated outputs would pass any tolerance
  m = fg_model.get_model(opt).load_weights(P)
  names = ['y_out', 'd_out'] if ref['d_out'] is not None else ['y_out']
  out = m.run(names, {'x': x, 'phase_train': False}, as_numpy=True)
  for n, got in zip(names, out):
    err = np.abs(got - ref[n]).max()
    print('%s %s: max|got - ref| = %.3g (span %.3f)' % (name, n, err, np.ptp(ref[n])))
    assert got.shape == ref[n].shape and err < TOL, (name, n, err)
  # 11. the 8-bit round trip
  y, d = m.prestage(x, quantise=True)
  _check_quantised(y.cpu().numpy(), ref['y_out'])
  if d is not None:
    _check_quantised(d.cpu().numpy(), ref['d_out'])
  else:
    assert ref['d_out'] is None
  single = m.run('y_out', {'x': torch.from_numpy(x), 'phase_train': False})
  assert isinstance(single, torch.Tensor) and single.is_cuda and np.array_equal(single.cpu().numpy(), out[0])


# ---- 12. / 13. chained into the decode loop
def _small_fg_opt():
  return dict(inp_depth=3, cnn_filter_size=[3] * 4, cnn_depth=[8, 16, 144, 32], cnn_pool=[1, 2, 2, 1],
              cnn_skip_mask=[True, False, True, False], dcnn_filter_size=[3] * 4, dcnn_depth=[160, 16, 8, 9], dcnn_pool=[2, 1, 2, 1],
              dcnn_skip_mask=[False, True, True], use_bn=True, add_skip_conn=True, add_orientation=True, num_orientation_classes=8,
              num_semantic_classes=1, weight_decay=5e-5)


def test_prestage_into_the_engine_is_the_fed_forward(cuda):
  import full_model
  fopt = _small_fg_opt()
  fg = fg_model.get_model(fopt).load_weights(fo.random_weights(fopt, 31))
  opt = ora.make_opt('kitti', 64, 96, 3)  # cfg3's architecture: add_d_out, add_y_out
  m = full_model.get_model(opt).load_weights(ora.random_params(opt, 4))
  assert m.dims['add_d_out'] and m.dims['add_y_out']
  x = np.random.RandomState(7).rand(2, 64, 96, 3).astype(np.float32)
  y_in, d_in = fg.prestage(x)
  y_in, d_in = y_in.clone(), d_in.clone()
  fed = [t.clone() for t in m.run(['y_out', 's_out'], {'x': x, 'y_in': y_in, 'd_in': d_in, 'phase_train': False})]
  eng = m.engine
  for _ in range(2):  # the second run replays the captured graph
    eng.glob['d_in'].zero_(), eng.glob['y_in'].zero_()
    for sb in eng.subs:
      sb['img'].fill_(3.0), sb['canvas'].fill_(3.0)
    y2, d2 = fg.prestage(x, into=eng)
    assert torch.equal(y2, y_in) and torch.equal(d2, d_in)
    eng.forward(x, prepacked=True).check_status()
    got = [m._fetch(n, eng) for n in ('y_out', 's_out')]
    assert torch.equal(got[0], fed[0]) and torch.equal(got[1], fed[1])
  # and the plain path is as it was
  again = m.run(['y_out', 's_out'], {'x': x, 'y_in': y_in, 'd_in': d_in, 'phase_train': False})
  assert torch.equal(again[0], fed[0]) and torch.equal(again[1], fed[1])


def test_command_lines(cuda, tmp_path):
  import yaml
  import fg_model_pack
  import full_model_eval
  res = str(tmp_path / 'results')
  fopt = _small_fg_opt()
  os.makedirs(os.path.join(res, 'fg'))
  with open(os.path.join(res, 'fg', 'model_opt.yaml'), 'w') as f:
    yaml.safe_dump(fopt, f)
  np.savez(os.path.join(res, 'fg', 'weights.npz'), step=np.float32(1), **fo.random_weights(fopt, 31))
  opt = ora.make_opt('kitti', 64, 96, 3)
  os.makedirs(os.path.join(res, 'full'))
  with open(os.path.join(res, 'full', 'model_opt.yaml'), 'w') as f:
    yaml.safe_dump({k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in opt.items()}, f)
  import full_model
  np.savez(os.path.join(res, 'full', 'weights.npz'), **full_model.get_model(opt).load_weights(ora.random_params(opt, 4)).state_dict_numpy())
  src, packed = str(tmp_path / 'in.npz'), str(tmp_path / 'out.npz')
  np.savez(src, x=np.random.RandomState(9).rand(5, 64, 96, 3).astype(np.float32))
  fg_model_pack.main(['--model_id', 'fg', '--results', res, '--input', src, '--output', packed, '--batch_size', '2'])
  out = dict(np.load(packed))
  assert out['y_in'].shape == (5, 64, 96, 1) and out['d_in'].shape == (5, 64, 96, 8) and out['y_in'].dtype == np.float32
  for k in ('y_in', 'd_in'):
    v = out[k] * np.float32(255)
    assert (v == np.round(v)).all() and np.ptp(out[k]) > 0.05
  assert (out['x'] == np.load(src)['x']).all()
  a, b = str(tmp_path / 'a'), str(tmp_path / 'b')
  full_model_eval.main(['--model_id', 'full', '--results', res, '--input', packed, '--output', a, '--batch_size', '2', '--test'])
  full_model_eval.main(['--model_id', 'full', '--results', res, '--input', src, '--output', b, '--batch_size', '2', '--test',
                        '--fg_model_id', 'fg'])
  da = [os.path.join(a, n) for n in os.listdir(a)][0]
  db = [os.path.join(b, n) for n in os.listdir(b)][0]
  ra, rb = np.load(os.path.join(da, 'pred_rank0.npz')), np.load(os.path.join(db, 'pred_rank0.npz'))
  assert ra['y_out'].shape == (5, 3, 64, 96)
  assert (ra['y_out'] == rb['y_out']).all() and (ra['s_out'] == rb['s_out']).all()
