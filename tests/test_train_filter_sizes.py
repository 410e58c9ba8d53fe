"""Training with filter sizes 1, 5 and 7 (model_opt['train_any_filter'], csrc/ra_wgrad_kxk.hip; nnlib.py:131-257, :260-404) — the
host side, no GPU: the new entries and their refusals, the opt-in guard of the trainers, the closures and the command lines, the
differentiable reference the GPU tests use, and the conditioning of the whole-step test's inputs."""
import ctypes as C

import numpy as np
import pytest
import torch

import box_model
import full_model
import nnlib as nn
import ra_native as rn
import ra_oracle as ora
import ra_oracle_torch as ort
import ra_train
import train_filter_cases as tfc
from ra_native import RecAttendError
from test_filter_sizes import mixed_opt

ENTRIES = ('ra_convkxk_wgrad_workspace_floats', 'ra_convkxk_wgrad_plan', 'ra_convkxk_wgrad_f32', 'ra_convkxk_wgrad_acc_f32',
           'ra_conv_pack_weights_k_dev', 'ra_subsample_even_f32')


def _ptr(a):
  return a.ctypes.data_as(C.c_void_p)


def test_entries_are_in_the_header_and_the_binding():
  lib = rn.lib()
  for name in ENTRIES:
    assert name in rn.SIGNATURES and hasattr(lib, name), name
  res, args = rn.SIGNATURES['ra_convkxk_wgrad_f32']
  assert res is C.c_int and len(args) == 14 and args[8] is C.c_int and args[10] is C.c_size_t
  assert len(rn.SIGNATURES['ra_convkxk_wgrad_acc_f32'][1]) == 17
  assert rn.SIGNATURES['ra_convkxk_wgrad_workspace_floats'][0] is C.c_size_t
  text = open(rn.HEADER_PATH).read()
  assert 'ra_convkxk_wgrad_f32 / _acc_f32' in text and 'nnlib.py:131-257, :260-404; csrc/ra_wgrad_kxk.hip' in text


@pytest.mark.parametrize('kf,cin,cout', [(0, 8, 8), (2, 8, 8), (4, 8, 8), (9, 8, 8), (5, 6, 8), (7, 8, 129), (1, 8, 200), (5, 0, 8)])
def test_entries_refuse_a_shape_without_a_launch(kf, cin, cout):
  """Host pointers: a refusal that came after a launch, or one that read the buffers' contents as addresses, would fault."""
  lib = rn.lib()
  buf = np.zeros(4096, np.float32)
  cm = np.zeros(64, np.int32)
  assert lib.ra_convkxk_wgrad_workspace_floats(kf, cin, cout, 2, 8, 8) == 0
  rc = lib.ra_convkxk_wgrad_f32(_ptr(buf), cin, 1, 8, 8, 0, _ptr(buf), cout, kf, _ptr(buf), 4096, _ptr(buf), _ptr(buf), None)
  assert rc == rn.RA_E_SHAPE, lib.ra_last_error_string()
  rc = lib.ra_convkxk_wgrad_acc_f32(_ptr(buf), cin, 1, 8, 8, 1, _ptr(buf), cout, kf, _ptr(buf), 4096, _ptr(cm), 4, 1, _ptr(buf), _ptr(buf),
                                    None)
  assert rc == rn.RA_E_SHAPE, lib.ra_last_error_string()
  rec = (C.c_int * rn.RA_WGK_PLAN_INTS)()
  assert lib.ra_convkxk_wgrad_plan(kf, cin, cout, 2, 8, 8, rec) == rn.RA_E_SHAPE
  if kf not in (1, 3, 5, 7):
    assert lib.ra_conv_pack_weights_k_dev(_ptr(buf), kf, 8, 8, 8, None, 0, _ptr(buf), None) == rn.RA_E_SHAPE


def test_workspace_and_plan_of_served_shapes():
  import ra_ops as ops
  lib = rn.lib()
  assert lib.ra_convkxk_wgrad_workspace_floats(3, 16, 32, 2, 9, 33) == lib.ra_conv3x3_wgrad_workspace_floats(16, 32, 2, 9, 33)
  for kf in tfc.SIZES:
    for cin, cout, nt in [(4, 8, 1), (8, 1, 1), (20, 16, 1), (16, 48, 2), (32, 128, 2), (40, 96, 2)]:
      p = ops.wgrad_kxk_plan(kf, cin, cout, 2, 9, 33)
      assert p['nt'] == nt and p['grid_y'] == -(-cin // 16) and p['grid_z'] == kf * ops.cout_padded(cout) // (16 * nt)
      assert p['ntiles'] == 8 and 1 <= p['grid_x'] <= 8 and p['acc_tiles'] == (kf + 1) * nt
      assert p['record_floats'] == (kf + 1) * 16 * 16 * nt and p['lds_bytes'] <= 64 * 1024
      assert lib.ra_convkxk_wgrad_workspace_floats(kf, cin, cout, 2, 9, 33) == p['grid_x'] * p['grid_y'] * p['grid_z'] * p['record_floats']


def test_train_any_filter_lifts_the_guard_and_nothing_else(monkeypatch):
  monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
  m = full_model.get_model(mixed_opt(train_any_filter=True))
  with pytest.raises(RecAttendError, match='needs an MI355X'):
    ra_train.TrainStep(m)
  b = box_model.get_model(mixed_opt('kitti', 64, 96, 2, train_any_filter=True))
  with pytest.raises(RecAttendError, match='needs an MI355X'):
    ra_train.BoxTrainStep(b)
  # without the key the refusal stands, and now names the flag
  with pytest.raises(RecAttendError, match='3x3.*train_any_filter'):
    ra_train.TrainStep(full_model.get_model(mixed_opt()))
  with pytest.raises(RecAttendError, match='3x3'):
    ra_train.TrainStep(full_model.get_model(mixed_opt(train_any_filter=False)))
  # with it, still refused by name: bf16 together with a non-3 layer, and such a layer with more than 128 channels
  with pytest.raises(RecAttendError, match="compute_dtype = 'bf16'"):
    ra_train.TrainStep(full_model.get_model(mixed_opt(train_any_filter=True, compute_dtype='bf16')))
  wide = mixed_opt(train_any_filter=True)
  wide['attn_cnn_depth'] = list(wide['attn_cnn_depth'])
  wide['attn_cnn_depth'][4] = 144  # the 7x7 layer
  with pytest.raises(RecAttendError, match='more than 128 channels'):  # the model itself refuses such a layer
    full_model.get_model(wide)
  with pytest.raises(RecAttendError, match='up to 128 channels'):  # ... and the trainers' guard a wide INPUT of one (its data gradient)
    ra_train._check_filter_sizes(dict(ccnn_filters=[3, 5], ccnn_channels=[4, 144, 64]), dict(train_any_filter=True), ('ccnn_filters',))
  assert ra_train._check_filter_sizes(dict(ccnn_filters=[3, 3], ccnn_channels=[4, 144, 64]), dict(train_any_filter=True), ('ccnn_filters',)) is False
  # an all-3x3 bf16 model with the key passes the guard: the key only matters where a layer differs from 3
  with pytest.raises(RecAttendError, match='needs an MI355X'):
    ra_train.TrainStep(full_model.get_model(ora.make_opt('cvppp', 64, 64, 2, train_any_filter=True, compute_dtype='bf16')))


def test_closures_take_the_keyword():
  """The refusal of the closures' training branch comes before they look at the input: with the keyword a CPU tensor gets
  past it and stops at the device check of the layer."""
  x = torch.zeros(1, 8, 8, 4)
  run = nn.cnn([5], [4, 8], [1], [nn.relu], [True], phase_train=True, train_any_filter=True)
  with pytest.raises(Exception) as e:
    run(x)
  assert '3x3' not in str(e.value)
  rund = nn.dcnn([1], [8, 4], [2], [nn.relu], [True], phase_train=True, train_any_filter=True)
  with pytest.raises(Exception) as e:
    rund(torch.zeros(1, 8, 8, 8))
  assert '3x3' not in str(e.value)
  with pytest.raises(RecAttendError, match='3x3.*train_any_filter=True'):
    nn.cnn([5], [4, 8], [1], [nn.relu], [True], phase_train=True)(x)
  # wide layers stay refused with the keyword
  with pytest.raises(RecAttendError, match='output channels is not built'):
    nn.cnn([3], [4, 192], [1], [nn.relu], [True], phase_train=True, train_any_filter=True)(x)


def test_cli_flag():
  import box_model_train
  import full_model_train
  for mod in (full_model_train, box_model_train):
    p = mod.build_parser()
    assert p.parse_args([]).train_any_filter is False and p.parse_args(['--train_any_filter']).train_any_filter is True
    assert 'train_any_filter' not in mod.make_opt(p.parse_args([]))  # model_opt.yaml of a default run is what it was
    opt = mod.make_opt(p.parse_args(['--train_any_filter', '--ctrl_cnn_filter_size', '5,3,1,3,7']))
    assert opt['train_any_filter'] is True and list(opt['ctrl_cnn_filter_size']) == [5, 3, 1, 3, 7]


@pytest.mark.parametrize('kf', [1, 3, 5, 7])
@pytest.mark.parametrize('H,W', [(3, 5), (4, 4)])
def test_deconv_reference_is_the_oracles_conv2d_transpose(kf, H, W):
  rng = np.random.RandomState(10 * kf + H)
  x, w, b = rng.randn(2, H, W, 3), rng.randn(kf, kf, 4, 3), rng.randn(4)
  for stride in (1, 2):
    got = tfc.deconv_ref(torch.tensor(x), torch.tensor(w), torch.tensor(b), stride).numpy()
    ref = ora.conv2d_transpose(x, w, stride) + b
    assert got.shape == ref.shape and np.abs(got - ref).max() < 1e-12, (kf, stride)
  if kf == 3:  # the oracle's own helper is this one at the size it was written for
    assert np.abs(ort.deconv_same(torch.tensor(x), torch.tensor(w), torch.tensor(b), 2).numpy() - got).max() < 1e-12


def test_wgrad_references_agree():
  """The einsum (plain conv) and the autograd of the transposed conv (upsample) are the same sum where both apply: a stride-1
  transposed conv is the plain conv of the flipped, in / out swapped filter."""
  rng = np.random.RandomState(2)
  x, du = torch.tensor(rng.randn(2, 5, 6, 4)), torch.tensor(rng.randn(2, 5, 6, 3))
  for kf in (1, 5, 7):
    dw, db = tfc.wgrad_ref(x, du, kf)
    w = torch.zeros((kf, kf, 3, 4), dtype=torch.float64, requires_grad=True)
    (tfc.deconv_ref(x, w, torch.zeros(3, dtype=torch.float64), 1) * du).sum().backward()
    assert np.abs(w.grad.flip(0, 1).permute(0, 1, 3, 2).numpy() - dw.numpy()).max() < 1e-10
    # the zero-stuffed statement of the kernel: X[2i + 1] = x[i] read through the window origin KF - 2 - pad_lo
    xs, dus = torch.tensor(rng.randn(1, 3, 5, 4)), torch.tensor(rng.randn(1, 6, 10, 3))
    ref, _ = tfc.wgrad_ref_ups(xs, dus, kf)
    org = kf - 2 - tfc.pad_lo(kf)
    z = torch.zeros((1, 6 + 2 * kf + 2, 10 + 2 * kf + 2, 4), dtype=torch.float64)  # U at offset kf + 1: room for every window
    z[:, kf + 2:kf + 2 + 6:2, kf + 2:kf + 2 + 10:2] = xs
    o = kf + 1 - org
    mine = torch.stack([torch.stack([torch.einsum('bhwc,bhwd->cd', z[:, o + ky:o + ky + 6, o + kx:o + kx + 10], dus)
                                     for kx in range(kf)]) for ky in range(kf)])
    assert np.abs(mine.numpy() - ref.numpy()).max() < 1e-10, kf


def test_step_inputs_are_well_conditioned(monkeypatch):
  """The precondition of the whole-step GPU test: on its inputs (train_filter_cases.step_case: a filter of size f scaled by
  3 / f) a float32 CPU run of the oracle itself meets, against its float64 run, the bars the kernels are held to."""
  from test_train_gpu import _compare_grads
  monkeypatch.setattr(ort, 'deconv_same', tfc.deconv_ref)
  opt, P, x, y_gt, s_gt = tfc.step_case()
  head64, g64, st64 = tfc.oracle_grads(opt, P, x, y_gt, s_gt)
  ort.set_dtype(torch.float32)
  try:
    head32, g32, st32 = tfc.oracle_grads(opt, P, x, y_gt, s_gt)
  finally:
    ort.set_dtype(torch.float64)
  for k in ('loss', 'iou_soft', 'iou_soft_box', 'conf_loss'):
    a, b = float(head32[k].detach()), float(head64[k].detach())
    assert abs(a - b) < 2e-4 * max(1.0, abs(b)), k
  assert (head32['match'].numpy() == head64['match'].numpy()).all()
  for key, (mean, var) in st64.items():
    rel = lambda a, b: float(np.abs(a - b).max() / max(1e-7, np.abs(b).max()))
    assert rel(st32[key][0].double().numpy(), mean.numpy()) < 1e-3 and rel(st32[key][1].double().numpy(), var.numpy()) < 1e-3, key
  wd = float(opt['weight_decay'])
  # _compare_grads adds wd * w to a decayed tensor's gradient (the product's optimizer kernel does): the oracle's has it already
  cos, worst = _compare_grads(g64, lambda k: g32[k] - (wd * P[k] if ra_train.is_decayed(k) else 0.0), P, wd)
  print('float32 oracle against float64 oracle: gradient cosine %.6f, worst per-tensor relative error %.4f' % (cos, worst))
