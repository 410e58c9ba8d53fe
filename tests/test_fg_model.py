"""fg_model at eval, the parts that need no GPU: the two oracles of tests/fg_oracle.py against each other, the shapes
get_model registers for the nets of run_kitti.sh / run_cityscapes.sh, the checkpoint names, the refusals, and the wide
layer's weight packing against its order written down in NumPy."""
import numpy as np
import pytest
import torch

import fg_model
import fg_oracle as fo
import nnlib
import ra_native as rn
import ra_ops as ops
from ra_native import RecAttendError


# ---- 1. the oracles pin each other
@pytest.mark.parametrize('nsc,ori', [(1, True), (9, True), (1, False), (3, False)])
def test_oracles_agree(nsc, ori):
  opt = fo.reduced_opt(nsc=nsc, orientation=ori)
  P = fo.random_weights(opt, 10 + nsc)
  x = np.random.RandomState(3).rand(2, 16, 24, 3)
  a, b = fo.forward(opt, P, x), fo.forward_torch(opt, P, x)
  for k in ('logits', 'y_out', 'd_out'):
    if a[k] is None:
      assert b[k] is None and not ori
      continue
    assert a[k].shape == b[k].shape and a[k].dtype == np.float64
    assert np.abs(a[k] - b[k]).max() < 1e-9, k
  assert a['y_out'].shape == (2, 16, 24, nsc)
  assert np.ptp(a['y_out']) > 0.05  # not a constant


def test_oracle_quantise_is_the_8_bit_round_trip():
  v = np.array([0.0, 0.5, 1.0, 0.9999, 1.0 / 255, 0.00391], np.float64)
  q = fo.quantise(v)
  assert q.dtype == np.float32
  assert (q * 255 == np.array([0, 127, 255, 254, 1, 0], np.float32)).all()


# ---- 2. shapes of the two run-script nets
KITTI_IN = [512, 512, 256, 256, 128, 192, 96, 64, 64, 32, 35]
CITY_IN = [512, 1024, 512, 512, 256, 384, 192, 256, 128, 192, 96, 67, 64]


@pytest.mark.parametrize('make,widths', [(fo.kitti_opt, KITTI_IN), (fo.cityscapes_opt, CITY_IN)])
def test_get_model_registers_the_reference_shapes(make, widths):
  opt = make()
  assert fo.dcnn_in_widths(opt) == widths
  m = fg_model.get_model(opt)
  cnn_ch = [3] + opt['cnn_depth']
  for i in range(len(opt['cnn_depth'])):
    assert tuple(m['cnn_w_%d' % i].shape) == (3, 3, cnn_ch[i], cnn_ch[i + 1])
    assert tuple(m['cnn_b_%d' % i].shape) == (cnn_ch[i + 1],)
  dch = [cnn_ch[-1]] + opt['dcnn_depth']
  for i in range(len(opt['dcnn_depth'])):
    assert tuple(m['dcnn_w_%d' % i].shape) == (3, 3, dch[i + 1], widths[i])
  assert m.dims['dcnn_in_ch'] == widths
  last = len(opt['dcnn_depth']) - 1
  assert 'dcnn_%d_0_gamma' % last not in m and 'dcnn_%d_0_gamma' % (last - 1) in m  # the last layer has no BN
  # 3. the checkpoint names
  shapes = fo.weight_shapes(opt)
  assert m.weight_keys() == sorted(shapes)
  sd = m.state_dict_numpy()
  assert {k: v.shape for k, v in sd.items()} == shapes


def test_cnn_filter_sizes_are_forced_to_3():
  m = fg_model.get_model(fo.reduced_opt())  # asks for 5
  assert all(tuple(m['cnn_w_%d' % i].shape[:2]) == (3, 3) for i in range(5))


def test_load_weights_strict_and_round_trip():
  opt = fo.reduced_opt(nsc=3, orientation=True)
  P = fo.random_weights(opt, 5)
  m = fg_model.get_model(opt)
  m.load_weights(dict(P, step=np.float32(40000)))  # `step` is accepted and ignored
  sd = m.state_dict_numpy()
  assert sorted(sd) == sorted(P)
  for k in P:
    assert (sd[k] == P[k]).all(), k
  assert (m['cnn_1_0_ema_var'].cpu().numpy() == P['cnn/layer_1/bn/ema_var']).all()
  m2 = fg_model.get_model(opt).load_weights(sd)
  assert all((m2.state_dict_numpy()[k] == P[k]).all() for k in P)
  miss = dict(P)
  del miss['dcnn/layer_2/bn/ema_mean']
  with pytest.raises(RecAttendError, match='missing'):
    fg_model.get_model(opt).load_weights(miss)
  bad = dict(P)
  bad['cnn/layer_0/w'] = np.zeros((3, 3, 4, 8), np.float32)
  with pytest.raises(RecAttendError, match='shape'):
    fg_model.get_model(opt).load_weights(bad)


# ---- 4. refusals, none of which needs a device
def test_refusals():
  opt = fo.reduced_opt()
  bad = dict(opt, dcnn_depth=opt['dcnn_depth'][:-1] + [7])
  with pytest.raises(RecAttendError, match='last dcnn channel'):
    fg_model.get_model(bad)
  m = fg_model.get_model(opt)
  x = np.zeros((1, 16, 16, 3), np.float32)
  with pytest.raises(RecAttendError, match='eval only'):
    m.run(['y_out'], {'x': x, 'phase_train': True})
  for name in ('loss', 'iou_soft', 'train_step'):
    with pytest.raises(RecAttendError, match='eval only'):
      m.run([name], {'x': x, 'phase_train': False})
  with pytest.raises(RecAttendError, match='multiples of the net\'s total pooling factor 4'):
    m.run(['y_out'], {'x': np.zeros((1, 18, 16, 3), np.float32), 'phase_train': False})
  wide5 = dict(opt, cnn_depth=[8, 16, 16, 24, 256], dcnn_depth=[256, 16, 12, 8, 9], dcnn_filter_size=[5, 3, 3, 3, 3])
  with pytest.raises(RecAttendError, match='3x3 filters only'):
    fg_model.get_model(wide5)


# ---- 5. packing of the wide layer
def _pack_ref(w, cin, cout, cmap, transposed):
  """[slice = co / 64][chunk = c / 16][tap = 3 ky + kx][ksub][n = co % 64][cg], kernel channel c = 16 chunk + 4 cg + ksub;
  transposed filters [3,3,Co,Ci] are flipped and read in/out-swapped; zero past Cin, Cout and where the map says -1."""
  ns, nc = -(-cout // 64), -(-cin // 16)
  out = np.zeros((ns, nc, 9, 4, 64, 4), np.float32)
  for c in range(cin):
    src = c if cmap is None else cmap[c]
    if src < 0:
      continue
    for ky in range(3):
      for kx in range(3):
        row = w[2 - ky, 2 - kx, :, src] if transposed else w[ky, kx, src, :]
        for co in range(cout):
          out[co // 64, c // 16, 3 * ky + kx, c % 4, co % 64, (c % 16) // 4] = row[co]
  return out.reshape(-1)


def test_pack_wide_weights():
  rng = np.random.RandomState(0)
  w = rng.randn(3, 3, 20, 144).astype(np.float32)
  assert (ops.pack_wide_weights(w) == _pack_ref(w, 20, 144, None, False)).all()
  assert rn.lib().ra_conv_wide_packed_floats(20, 144) == 3 * 2 * 9216
  # transposed, with a channel map: prev 10 channels padded to 12, skip 3 padded to 4
  wt = rng.randn(3, 3, 192, 13).astype(np.float32)
  cmap = list(range(10)) + [-1, -1] + [10, 11, 12, -1]
  got = ops.pack_wide_weights(wt, cin_kernel=16, chan_map=cmap, transposed=True)
  assert (got == _pack_ref(wt, 16, 192, cmap, True)).all()
  # pack_conv_weights sends such a filter the same way
  assert (ops.pack_conv_weights(wt, cin_kernel=16, chan_map=cmap, transposed=True) == got).all()
  lib = rn.lib()
  for cin, cout in ((256, 512), (1024, 512), (512, 256), (192 + 192, 192)):
    assert lib.ra_conv_wide_supported(cin, cout) == 1 and ops.conv_wide_supported(cin, cout)
  assert lib.ra_conv_wide_supported(512, 520) == 0 and lib.ra_conv_wide_supported(1028, 512) == 0
  assert lib.ra_conv_wide_supported(64, 128) == 0 and lib.ra_conv_wide_supported(66, 256) == 0
  assert lib.ra_conv_wide_packed_floats(512, 520) == 0
  assert lib.ra_conv_cout_padded(129) == 0  # K1 itself is as it was
  # unsupported shapes are refused before any launch
  rc = lib.ra_conv3x3_wide_f32(1, 512, None, 0, 1, 8, 8, 0, 1, 1, 1, 520, 1, 1, 1, None)
  assert rc == rn.RA_E_SHAPE
  rc = lib.ra_fg_head_f32(1, 16, 17, 8, 0, 1, 1, None, 0, None, 0, None, None)
  assert rc != 0 and b'nsc' in lib.ra_last_error_string()
  with pytest.raises(RecAttendError):
    ops.pack_wide_weights(rng.randn(3, 3, 8, 520).astype(np.float32))
  with pytest.raises(RecAttendError, match='3x3'):
    ops.pack_conv_weights(rng.randn(5, 5, 8, 256).astype(np.float32))


def test_fold_bn_of_a_wide_layer():
  rng = np.random.RandomState(1)
  b = rng.randn(256).astype(np.float32)
  bn = tuple(a.astype(np.float32) for a in (rng.randn(256), rng.rand(256) + 0.5, rng.randn(256), rng.rand(256) + 0.5))
  sc, sh = ops.fold_bn(b, 256, bn)
  sc128, sh128 = ops.fold_bn(b[:128], 128, tuple(a[:128] for a in bn))  # the library's own fold
  assert sc.shape == (256,) and np.allclose(sc[:128], sc128, rtol=3e-7, atol=0) and np.allclose(sh[:128], sh128, rtol=0, atol=1e-6)
  sc, sh = ops.fold_bn(b, 256, None)
  assert (sc == 1).all() and (sh == b).all()


# ---- 6. training with a wide layer
def test_training_with_a_wide_layer_is_refused():
  run = nnlib.cnn([3], [64, 256], [1], [nnlib.relu], [True], phase_train=True, model={})
  with pytest.raises(RecAttendError, match='training with layers of .* output channels is not built'):
    run(torch.zeros(1, 8, 8, 64))
  run = nnlib.dcnn([3], [64, 256], [2], [nnlib.relu], [True], phase_train=True, model={})
  with pytest.raises(RecAttendError, match='training with layers of .* output channels is not built'):
    run(torch.zeros(1, 8, 8, 64))
