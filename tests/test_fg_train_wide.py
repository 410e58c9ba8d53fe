"""Training fg_model's wide layers, the parts that need no device: the argument checks of the new entry points (host pointers:
nothing is dereferenced, nothing is launched), the wide filter gradient's plan and workspace queries, the opt-in form checks of
ra_fg_train for the nets of the reference's run scripts, and the command line's --train_wide."""
import ctypes as C

import pytest
import torch

import fg_model
import fg_model_train
import fg_oracle as fo
import ra_fg_train
import ra_native as rn
import ra_ops as ops
from ra_native import RecAttendError

# (Cin, Cout, B, Hs, Ws, upsample) of tests/test_wgrad_wide_gpu.py (spelled out: importing a GPU test module is not needed here)
GPU_CASES = [(4, 144, 1, 5, 7, 0), (20, 144, 2, 5, 7, 0), (132, 272, 2, 8, 16, 0), (64, 192, 2, 4, 8, 1), (272, 512, 1, 3, 5, 1),
             (1024, 512, 2, 4, 8, 0), (192, 192, 2, 32, 64, 0), (144, 144, 3, 24, 24, 0)]
BIG = 1 << 40


def test_wide_wgrad_entry_refuses_bad_arguments():
  lib = rn.lib()
  ok = dict(x=1, cin=64, B=2, Hs=8, Ws=8, ups=0, du=1, cout=192, ws=1, nws=BIG, cmap=None, cin_w=64, tr=0, gw=1, gb=None)

  def call(**kw):
    a = dict(ok, **kw)
    return lib.ra_conv3x3_wgrad_wide_acc_f32(a['x'], a['cin'], a['B'], a['Hs'], a['Ws'], a['ups'], a['du'], a['cout'], a['ws'], a['nws'],
                                             a['cmap'], a['cin_w'], a['tr'], a['gw'], a['gb'], None)

  for bad in (dict(x=None), dict(du=None), dict(ws=None), dict(gw=None), dict(B=0), dict(Hs=0), dict(Ws=-1), dict(cin=0), dict(cin_w=0),
              dict(cin_w=65)):  # more filter rows than kernel channels without a map
    assert call(**bad) == rn.RA_E_INVALID, bad
    assert b'ra_conv3x3_wgrad_wide_acc_f32' in lib.ra_last_error_string()
  for bad in (dict(cout=128), dict(cout=130), dict(cout=528), dict(cout=64), dict(cin=6, cin_w=6), dict(cin=1028)):
    assert call(**bad) == rn.RA_E_SHAPE, bad
  need = lib.ra_conv3x3_wgrad_wide_workspace_floats(64, 192, 2, 8, 8)
  assert need > 0 and call(nws=need - 1) == rn.RA_E_WORKSPACE
  assert call(ups=1, nws=need) == rn.RA_E_WORKSPACE  # the map is twice the size: more pixel tiles, more parts
  for bad in ((6, 192), (64, 130), (64, 128), (1028, 512)):
    assert lib.ra_conv3x3_wgrad_wide_workspace_floats(bad[0], bad[1], 2, 8, 8) == 0
  rec = (C.c_int * rn.RA_WGW_PLAN_INTS)()
  assert lib.ra_conv3x3_wgrad_wide_plan(64, 192, 2, 8, 8, 0, None) == rn.RA_E_INVALID
  assert lib.ra_conv3x3_wgrad_wide_plan(64, 192, 0, 8, 8, 0, rec) == rn.RA_E_INVALID
  assert lib.ra_conv3x3_wgrad_wide_plan(64, 130, 2, 8, 8, 0, rec) == rn.RA_E_SHAPE
  assert lib.ra_conv3x3_wgrad_wide_plan(6, 192, 2, 8, 8, 0, rec) == rn.RA_E_SHAPE


def test_wide_bn_entries_refuse_bad_arguments():
  lib = rn.lib()
  need = lib.ra_bn_wide_workspace_floats(192)
  assert need >= 2 * 192
  mom = lambda u=1, npix=64, C_=192, ws=1, nws=need, mean=1, var=1: lib.ra_bn_wide_moments_f32(u, npix, C_, ws, nws, mean, var, None)
  assert mom(u=None) == mom(ws=None) == mom(mean=None) == mom(var=None) == mom(npix=0) == mom(C_=0) == rn.RA_E_INVALID
  assert mom(C_=130) == mom(C_=516) == rn.RA_E_SHAPE
  assert mom(nws=need - 1) == rn.RA_E_WORKSPACE and b'ra_bn_wide_moments_f32' in lib.ra_last_error_string()
  fwd = lambda u=1, y=1, pool=1, H=6, W=10, C_=192: lib.ra_bn_wide_act_pool_f32(u, 1, 1, 1, 1, 1e-3, 1, pool, 2, H, W, C_, y, None)
  assert fwd(u=None) == fwd(y=None) == fwd(H=0) == rn.RA_E_INVALID
  assert fwd(C_=130) == fwd(C_=516) == fwd(pool=3) == fwd(pool=2, H=5) == rn.RA_E_SHAPE
  bwd = lambda u=1, dy=1, ws=1, nws=need, dg=1, db=1, du=1, pool=1, W=10, C_=192: lib.ra_bn_wide_act_pool_bwd_acc_f32(
      u, dy, 1, 1, 1, 1, 1e-3, 1, pool, 2, 6, W, C_, ws, nws, dg, db, du, None, None, None)
  assert bwd(u=None) == bwd(dy=None) == bwd(ws=None) == bwd(dg=None) == bwd(db=None) == bwd(du=None) == rn.RA_E_INVALID
  assert bwd(C_=132 + 2) == bwd(C_=1024) == bwd(pool=2, W=9) == rn.RA_E_SHAPE
  assert bwd(nws=need - 1) == rn.RA_E_WORKSPACE


def test_wide_pack_entry_refuses_bad_arguments():
  lib = rn.lib()
  pack = lambda w=1, cin_w=16, cout=544, cin=16, first=0, count=272, out=1: lib.ra_conv_wide_pack_weights_dev(w, cin_w, cout, cin, None, 0, first,
                                                                                                            count, out, None)
  assert pack(w=None) == pack(out=None) == pack(cin_w=0) == pack(first=-1) == pack(count=0) == rn.RA_E_INVALID
  assert pack(count=128) == pack(count=130) == pack(count=528) == pack(cin=6) == rn.RA_E_SHAPE  # the range obeys the wide conv's limits
  assert pack(first=288) == rn.RA_E_SHAPE and b'channels [288, 560) of 544' in lib.ra_last_error_string()
  assert pack(cin=20) == rn.RA_E_SHAPE  # a kernel input wider than the filter needs a map
  w = torch.zeros(3, 3, 16, 272)
  with pytest.raises(RecAttendError, match='no CPU fallback'):
    ops.pack_wide_weights_dev(w)
  with pytest.raises(RecAttendError, match='no CPU fallback'):
    ops.bn_wide_moments(torch.zeros(2, 4, 4, 192))
  with pytest.raises(RecAttendError, match='no CPU fallback'):
    ops.wgrad_wide_acc(torch.zeros(1, 8, 8, 64), torch.zeros(1, 8, 8, 192), torch.zeros(3, 3, 64, 192))


def test_wide_wgrad_plan_and_workspace():
  """The workspace query is the plan's answer; the GPU cases reach one part and several, a short last part, and the kernel's one
  tile form."""
  lib = rn.lib()
  plans = {}
  for cin, cout, B, Hs, Ws, ups in GPU_CASES:
    p = plans[(cin, cout, B, Hs, Ws, ups)] = ops.wgrad_wide_plan(cin, cout, B, Hs, Ws, ups)
    up = 1 + ups
    assert set(p) == {'tile_ci', 'tile_co', 'tile_pix', 'taps', 'grid_ci', 'grid_co', 'split', 'tiles_per_part', 'ntiles', 'lds', 'ws_floats'}
    assert (p['grid_ci'], p['grid_co']) == (-(-cin // p['tile_ci']), -(-cout // p['tile_co']))
    assert p['ntiles'] == B * -(-Hs * up // p['tile_pix']) * -(-Ws * up // p['tile_pix'])
    # every part has a tile, the last one may be short
    assert 1 <= p['split'] <= 64 and (p['split'] - 1) * p['tiles_per_part'] < p['ntiles'] <= p['split'] * p['tiles_per_part']
    cip, cop = p['grid_ci'] * p['tile_ci'], p['grid_co'] * p['tile_co']
    assert p['ws_floats'] == p['split'] * (9 * cip * cop + cop) == lib.ra_conv3x3_wgrad_wide_workspace_floats(cin, cout, B, Hs * up, Ws * up)
    assert p['lds'] <= 64 * 1024
  assert {(p['tile_ci'], p['tile_co'], p['tile_pix'], p['taps']) for p in plans.values()} == {(64, 64, 8, 9)}  # the chooser's one tile form
  splits = {k: p['split'] for k, p in plans.items()}
  assert splits[(1024, 512, 2, 4, 8, 0)] == 1 and splits[(4, 144, 1, 5, 7, 0)] == 1
  assert splits[(192, 192, 2, 32, 64, 0)] == 16 and plans[(192, 192, 2, 32, 64, 0)]['tiles_per_part'] == 4
  short = plans[(144, 144, 3, 24, 24, 0)]  # 27 tiles in parts of 5: the last has 2
  assert (short['split'], short['tiles_per_part'], short['ntiles']) == (6, 5, 27)
  # the run scripts' largest layers at their training shapes keep at least four tiles per part and at most 64 parts
  big = ops.wgrad_wide_plan(1024, 512, 8, 32, 64)
  assert big['split'] * big['grid_ci'] * big['grid_co'] >= 256 and big['tiles_per_part'] >= 4


def _trainer(opt, **kw):
  return ra_fg_train.FgTrainStep(fg_model.get_model(opt), **kw)


def _cli_default_with_skips():
  p = fg_model_train.build_parser()
  return fg_model_train.make_opt(p.parse_args(['--add_skip_conn', '--add_orientation', '--dcnn_depth', '128,128,64,64,32,32,16,16,8,8,9']))


def test_wide_form_checks_admit_the_run_script_nets():
  for opt in (fo.kitti_opt(), fo.cityscapes_opt(), _cli_default_with_skips(), fo.reduced_opt(wide=True)):
    d = fg_model.derive(opt)
    ra_fg_train.check_options(opt, d, wide=True)
    ra_fg_train.check_kernel_forms(d, wide=True)
  # ... and without the flag they answer as before, now naming it
  with pytest.raises(RecAttendError, match='is not built .*eval decodes.*wide=True'):
    ra_fg_train.check_options(fo.kitti_opt(), fg_model.derive(fo.kitti_opt()))
  with pytest.raises(RecAttendError, match='dcnn layer 2 .*192 channels is not built.*--train_wide'):
    ra_fg_train.check_kernel_forms(fg_model.derive(_cli_default_with_skips()))


def test_wide_form_checks_name_the_layer():
  opt = fo.reduced_opt(wide=True)  # cnn layer 3 has 144 channels and is the skip of dcnn layer 1 (16 + 144 -> 16)
  d = fg_model.derive(opt)
  d['dcnn_filter_size'][1] = 5
  with pytest.raises(RecAttendError, match='dcnn layer 1 .*filter size 5'):
    ra_fg_train.check_kernel_forms(d, wide=True)
  d = fg_model.derive(opt)
  d['cnn_channels'][4] = 130
  with pytest.raises(RecAttendError, match='cnn layer 3 .*multiple of 16'):
    ra_fg_train.check_kernel_forms(d, wide=True)
  d = fg_model.derive(opt)
  d['cnn_channels'][4] = 528
  with pytest.raises(RecAttendError, match='cnn layer 3 .*up to 512'):
    ra_fg_train.check_kernel_forms(d, wide=True)
  d = fg_model.derive(opt)
  d['cnn_channels'][3] = 18  # a source of the wide layer that is no multiple of 4
  with pytest.raises(RecAttendError, match='cnn layer 3 .*multiples of 4'):
    ra_fg_train.check_kernel_forms(d, wide=True)
  d = fg_model.derive(opt)
  d['dcnn_skip_ch'][1] = 136  # a data gradient of 136 channels: beyond K1 and no multiple of 16
  with pytest.raises(RecAttendError, match='dcnn layer 1 .*source of 136 channels'):
    ra_fg_train.check_kernel_forms(d, wide=True)
  with pytest.raises(RecAttendError, match="compute_dtype = 'bf16'"):
    ra_fg_train.check_options(dict(opt, compute_dtype='bf16'), fg_model.derive(opt), wide=True)
  # what is refused without the flag stays refused with it
  with pytest.raises(RecAttendError, match='dcnn_filter_size .* is not built'):
    _trainer(dict(opt, dcnn_filter_size=[3, 5, 3, 3, 3]), wide=True)
  with pytest.raises(RecAttendError, match='optimizer'):
    _trainer(dict(opt, optimizer='sgd'), wide=True)


def test_wide_trainer_needs_a_device(monkeypatch):
  monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
  monkeypatch.delenv('WORLD_SIZE', raising=False)
  with pytest.raises(RecAttendError, match='needs an MI355X'):
    _trainer(fo.kitti_opt(), wide=True)


def test_cli_has_train_wide():
  p = fg_model_train.build_parser()
  assert p.parse_args([]).train_wide is False and p.parse_args(['--train_wide']).train_wide is True
  assert 'train_wide' not in fg_model_train.make_opt(p.parse_args([]))  # model_opt.yaml of a default run is what it was
  opt = fg_model_train.make_opt(p.parse_args(['--train_wide', '--add_skip_conn']))
  assert opt['train_wide'] is True
  fg_model.derive(opt)  # an option the model ignores
