"""Filter sizes 1, 5 and 7 next to 3 in the cnn / dcnn layers (nnlib.py:131-257, :260-404) — the host side, no GPU:
models build with mixed sizes and round-trip their weights, the packer matches a NumPy restatement of its order,
other sizes and training with a size other than 3 are refused before any kernel runs."""
import ctypes as C

import numpy as np
import pytest
import torch

import box_model
import full_model
import nnlib as nn
import ra_native as rn
import ra_ops as ops
import ra_oracle as ora
import ra_train
from ra_native import RecAttendError

CTRL = [5, 3, 1, 3, 7, 3, 3, 3]
ATTN = [5, 3, 1, 3, 7, 3]
DCNN = [3, 5, 5, 7, 1, 3, 1]  # unpool [2, 1, 2, 1, 2, 1, 1]: stride 2 at 3 / 5 / 1, stride 1 at 5 / 7 / 3 / 1


def mixed_opt(arch='cvppp', H=64, W=64, T=2, **over):
  return ora.make_opt(arch, H, W, T, ctrl_cnn_filter_size=CTRL, attn_cnn_filter_size=ATTN,
                      attn_dcnn_filter_size=DCNN, **over)


def _ptr(a):
  return None if a is None else a.ctypes.data_as(C.c_void_p)


def test_full_model_builds_with_mixed_sizes_and_registers_f_by_f_filters():
  opt = mixed_opt()
  m = full_model.get_model(opt)
  d = m.dims
  assert (d['ccnn_filters'], d['acnn_filters'], d['adcnn_filters']) == (CTRL, ATTN, DCNN)
  for i, f in enumerate(CTRL):
    assert tuple(m['ctrl_cnn_w_%d' % i].shape) == (f, f, d['ccnn_channels'][i], d['ccnn_channels'][i + 1])
  for i, f in enumerate(ATTN):
    assert tuple(m['attn_cnn_w_%d' % i].shape) == (f, f, d['acnn_channels'][i], d['acnn_channels'][i + 1])
  for i, f in enumerate(DCNN):
    shp = tuple(m['attn_dcnn_w_%d' % i].shape)
    assert shp[:2] == (f, f) and shp[2] == d['adcnn_channels'][i + 1]
  sd = m.state_dict_numpy()
  m2 = full_model.get_model(opt).load_weights(sd)
  for k, v in m2.state_dict_numpy().items():
    assert np.array_equal(v, sd[k]), k
  # the shapes are checked against what is registered: a 3x3 filter does not load into a 5x5 layer
  bad = dict(sd)
  bad['ctrl_cnn_w_0'] = np.zeros((3, 3) + sd['ctrl_cnn_w_0'].shape[2:], np.float32)
  with pytest.raises(RecAttendError):
    full_model.get_model(opt).load_weights(bad)


def test_box_model_builds_with_mixed_sizes():
  opt = mixed_opt('kitti', 64, 96, 2)
  m = box_model.get_model(opt)
  for i, f in enumerate(CTRL):
    assert tuple(m['ctrl_cnn_w_%d' % i].shape[:2]) == (f, f)
  sd = m.state_dict_numpy()
  m2 = box_model.get_model(opt).load_weights(sd)
  assert all(np.array_equal(v, sd[k]) for k, v in m2.state_dict_numpy().items())


@pytest.mark.parametrize('f', [2, 4, 9, 0])
def test_other_filter_sizes_are_refused(f):
  with pytest.raises(RecAttendError, match='filter size %d' % f):
    full_model.get_model(ora.make_opt('cvppp', 64, 64, 2, ctrl_cnn_filter_size=[3, f] + [3] * 6))
  with pytest.raises(RecAttendError, match='filter size %d' % f):
    full_model.get_model(ora.make_opt('cvppp', 64, 64, 2, attn_dcnn_filter_size=[3] * 6 + [f]))
  with pytest.raises(RecAttendError, match='filter size %d' % f):
    nn.cnn([f], [4, 8], [1], [nn.relu], [False])
  with pytest.raises(RecAttendError):
    ops.pack_conv_weights(np.zeros((f, f, 4, 8), np.float32))
  lib = rn.lib()
  assert lib.ra_conv_packed_floats_k(f, 8, 8) == 0
  # the entry refuses the size before it looks at the (here: host) buffers or launches anything
  buf = np.zeros(4096, np.float32)
  rc = lib.ra_convkxk_f32(_ptr(buf), 4, None, 0, 1, 8, 8, 0, _ptr(buf), f, _ptr(buf), _ptr(buf), 8, 1, 1, None, -1,
                          _ptr(buf), None)
  assert rc == rn.RA_E_SHAPE
  assert ('filter size %d' % f).encode() in lib.ra_last_error_string()


def _chunk(kf, cin):
  if kf <= 3:
    return 16 if cin % 16 == 0 else 8 if cin % 8 == 0 else 4
  return 8 if kf == 5 and cin % 8 == 0 else 4


def _pack_ref(w, kf, cin, cmap, transposed):
  """NumPy restatement of the packed order [chunk][tap = ky*KF+kx][cg][ksub][CoutP], channel chunk*CK + 4*cg + ksub."""
  cout = w.shape[2] if transposed else w.shape[3]
  cp = ops.cout_padded(cout)
  ck = _chunk(kf, cin)
  out = np.zeros((cin // ck, kf * kf, ck // 4, 4, cp), np.float32)
  for c in range(cin):
    src = c if cmap is None else cmap[c]
    if src < 0:
      continue
    for ky in range(kf):
      for kx in range(kf):
        col = w[kf - 1 - ky, kf - 1 - kx, :, src] if transposed else w[ky, kx, src, :]
        out[c // ck, ky * kf + kx, (c % ck) // 4, c % 4, :cout] = col
  return out.reshape(-1)


@pytest.mark.parametrize('kf', [1, 3, 5, 7])
@pytest.mark.parametrize('transposed', [False, True])
@pytest.mark.parametrize('cin_w,cin,cout,mapped', [(4, 4, 8, False), (13, 16, 16, True), (16, 16, 1, False),
                                                   (24, 24, 32, False), (32, 32, 64, False), (20, 24, 96, True),
                                                   (96, 96, 64, False)])
def test_pack_weights_k_matches_numpy_order(kf, transposed, cin_w, cin, cout, mapped):
  rng = np.random.RandomState(kf * 100 + cin + cout)
  shp = (kf, kf, cout, cin_w) if transposed else (kf, kf, cin_w, cout)
  w = rng.randn(*shp).astype(np.float32)
  cmap = None
  if mapped:  # a permuted subset with zero (padding) channels, as the packed model input's map
    cmap = list(rng.permutation(cin_w)) + [-1] * (cin - cin_w)
    cmap[1] = -1
  lib = rn.lib()
  n = lib.ra_conv_packed_floats_k(kf, cin, cout)
  assert n == kf * kf * cin * ops.cout_padded(cout)
  out = np.full(n, np.nan, np.float32)
  cm = None if cmap is None else np.ascontiguousarray(cmap, np.int32)
  flags = rn.RA_CONV_TRANSPOSED if transposed else 0
  assert lib.ra_conv_pack_weights_k(_ptr(w), kf, cin_w, cout, cin, _ptr(cm), flags, _ptr(out)) == 0
  assert np.array_equal(out, _pack_ref(w, kf, cin, cmap, transposed))
  assert np.array_equal(ops.pack_conv_weights(w, cin_kernel=cin, chan_map=cmap, transposed=transposed), out)
  if kf == 3:  # bit-identical to the 3x3 packer
    old = np.full(lib.ra_conv_packed_floats(cin, cout), np.nan, np.float32)
    assert lib.ra_conv_pack_weights(_ptr(w), cin_w, cout, cin, _ptr(cm), flags, _ptr(old)) == 0
    assert old.tobytes() == out.tobytes()


def test_training_is_refused_for_other_sizes_before_any_kernel():
  opt = mixed_opt()
  m = full_model.get_model(opt)
  with pytest.raises(RecAttendError, match='3x3'):
    ra_train.TrainStep(m)
  b = box_model.get_model(mixed_opt('kitti', 64, 96, 2))
  with pytest.raises(RecAttendError, match='3x3'):
    ra_train.BoxTrainStep(b)
  # the closures' training branch refuses too (before it looks at the input)
  run = nn.cnn([5], [4, 8], [1], [nn.relu], [True], phase_train=True)
  with pytest.raises(RecAttendError, match='3x3'):
    run(torch.zeros(1, 8, 8, 4))
  rund = nn.dcnn([1], [8, 4], [2], [nn.relu], [True], phase_train=True)
  with pytest.raises(RecAttendError, match='3x3'):
    rund(torch.zeros(1, 8, 8, 8))
  # an all-3x3 model passes the guard
  m3 = full_model.get_model(ora.make_opt('cvppp', 64, 64, 2))
  ra_train._check_3x3(m3.dims, ('ccnn_filters', 'acnn_filters', 'adcnn_filters'))
