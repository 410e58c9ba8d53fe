"""End-to-end parity of the decode loop (full_model / box_model forward on MI355X, through
the C ABI) against the float64 NumPy oracle on the same seeded inputs and weights.
Bar: masks within 1e-3 max-abs (BASELINE.json north_star); observed ~1e-5."""
import numpy as np
import pytest
import torch

import ra_oracle as ora

pytestmark = pytest.mark.gpu

MASK_TOL = 1e-3  # the north star's tolerance on masks


def _inputs(opt, B, seed):
  rng = np.random.RandomState(seed)
  H, W = opt['inp_height'], opt['inp_width']
  x = rng.rand(B, H, W, 3).astype(np.float32)
  d_in = y_in = None
  if opt.get('add_d_out'):
    lab = rng.randint(0, 8, (B, H, W))
    d_in = np.eye(8, dtype=np.float32)[lab]
    logits = rng.randn(B, H, W, opt['num_semantic_classes'])
    y_in = ora.softmax(logits).astype(np.float32)
  return x, d_in, y_in


def _check(opt, B, seed, use_graph, tune=None, ref=None):
  import full_model
  P = ora.random_params(opt, seed)
  if tune is not None:
    P = tune(P)
  x, d_in, y_in = _inputs(opt, B, seed + 1)
  if ref is None:
    ref = ora.full_model_forward(opt, P, x, d_in, y_in)
  m = full_model.get_model(opt).load_weights(P)
  m.engine.use_graph = use_graph
  feed = {'x': x, 'phase_train': False, 'd_in': d_in, 'y_in': y_in}
  names = ['y_out', 's_out', 'x_patch', 'y_out_patch', 'attn_ctr', 'attn_size',
           'ctrl_rnn_glimpse_map', 'attn_box', 'canvas']
  for rep in range(2 if use_graph else 1):  # second pass = graph replay
    out = dict(zip(names, m.run(names, feed, as_numpy=True)))
    assert out['y_out'].shape == ref['y_out'].shape
    assert np.abs(out['attn_ctr'] - ref['attn_ctr']).max() < 2e-3
    assert np.abs(out['attn_size'] - ref['attn_size']).max() < 2e-3
    assert np.abs(out['ctrl_rnn_glimpse_map'] - ref['ctrl_rnn_glimpse_map']).max() < 1e-4
    assert np.abs(out['x_patch'] - ref['x_patch']).max() < 1e-3
    assert np.abs(out['y_out_patch'] - ref['y_out_patch']).max() < 1e-3
    assert np.abs(out['y_out'] - ref['y_out']).max() < MASK_TOL
    assert np.abs(out['s_out'] - ref['s_out']).max() < MASK_TOL
    assert np.abs(out['attn_box'] - ref['attn_box']).max() < MASK_TOL
    assert np.abs(out['canvas'] - ref['canvas']).max() < MASK_TOL
  return out, ref


def test_cfg1_cvppp_128(cuda):
  """BASELINE.json configs[0]: CVPPP full_model 128x128, 5 timesteps, batch 1."""
  out, ref = _check(ora.make_opt('cvppp', 128, 128, 5), 1, 16, use_graph=False)
  assert ref['y_out'].max() > 0.5  # the fixture is not a trivial all-sigma(-5) mask
  print('max |dy|', np.abs(out['y_out'] - ref['y_out']).max())


def test_cvppp_graph_replay_batch3(cuda):
  _check(ora.make_opt('cvppp', 128, 160, 3), 3, 14, use_graph=True)


def test_cvppp_disable_overwrite_and_no_fixed_gamma(cuda):
  _check(ora.make_opt('cvppp', 96, 96, 3, disable_overwrite=True, fixed_gamma=False), 2, 31, False)


def test_kitti_arch_skip_dynamic_var(cuda):
  """KITTI-style flags: skip connections, dynamic_var, 13 input channels."""
  _check(ora.make_opt('kitti', 64, 96, 3), 2, 41, use_graph=False)


def test_cityscapes_arch(cuda):
  _check(ora.make_opt('cityscapes', 64, 128, 2), 1, 51, use_graph=True)


def test_cfg3_kitti_native_size(cuda):
  """BASELINE.json configs[2] at the size the reference feeds the model (KITTI images
  are resized to 128x448, T=20): parity at B=2, then the configured B=16 (more images than the
  16-workgroup controller takes: the single-workgroup controller path) row-independent of it."""
  import full_model
  opt = ora.make_opt('kitti', 128, 448, 20)
  out, ref = _check(opt, 2, 61, use_graph=True)
  P = ora.random_params(opt, 61)
  x, d_in, y_in = _inputs(opt, 2, 62)
  rep = lambda a: np.concatenate([a] * 8)
  m = full_model.get_model(opt).load_weights(P)
  y16 = m.run('y_out', {'x': rep(x), 'd_in': rep(d_in), 'y_in': rep(y_in), 'phase_train': False}, as_numpy=True)
  assert y16.shape == (16, 20, 128, 448)
  assert np.abs(y16[:2] - out['y_out']).max() < 1e-4 and np.abs(y16[14:] - out['y_out']).max() < 1e-4


def test_cfg5_cityscapes_native_size(cuda):
  """BASELINE.json configs[4] at the model's native 256x512, T=20 (9 semantic classes, 21 input
  channels, skip connections, dynamic_var), one image against the oracle."""
  _check(ora.make_opt('cityscapes', 256, 512, 20), 1, 71, use_graph=True)


@pytest.mark.parametrize('over', [
    dict(num_ctrl_mlp_layers=2, ctrl_mlp_dim=64, num_glimpse_mlp_layers=3, num_ctrl_rnn_iter=3, ctrl_rnn_hid_dim=128),
    dict(filter_height=32, filter_width=32, squash_ctrl_params=True, fixed_var=True),
    dict(num_ctrl_rnn_iter=1, ctrl_rnn_hid_dim=64, fixed_gamma=False, dynamic_var=True),
], ids=['deep_mlps_small_lstm', 'patch32_squash_fixed_var', 'one_glimpse_dynamic_var'])
def test_option_corners(cuda, over):
  """model_opt values off the run scripts' beaten path: the generic controller / kernel variants."""
  _check(ora.make_opt('cvppp', 96, 128, 2, **over), 2, 81, use_graph=False)


def test_long_sequence_t32_and_loss_head(cuda):
  """T = 32 (the cfg5 T=32 variant's sequence length; the loss head's and matching's maximum),
  small image: decode parity, then the loss head against the oracle with 20 instances."""
  import full_model
  opt = ora.make_opt('cvppp', 64, 64, 32)
  out, ref = _check(opt, 1, 91, use_graph=True)
  rng = np.random.RandomState(92)
  yy, xx = np.mgrid[0:64, 0:64]
  y_gt, s_gt = np.zeros((1, 32, 64, 64), np.float32), np.zeros((1, 32), np.float32)
  for t in range(20):
    cy, cx = rng.randint(6, 58), rng.randint(6, 58)
    y_gt[0, t] = ((yy - cy) ** 2 + (xx - cx) ** 2 < 16)
    s_gt[0, t] = 1
  P = ora.random_params(opt, 91)
  x, _, _ = _inputs(opt, 1, 92)
  href = ora.loss_head(opt, ora.full_model_forward(opt, P, x), y_gt, s_gt)
  m = full_model.get_model(opt).load_weights(P)
  names = ['loss', 'iou_soft', 'conf_loss', 'dice', 'match']
  got = dict(zip(names, m.run(names, {'x': x, 'phase_train': False, 'y_gt': y_gt, 's_gt': s_gt}, as_numpy=True)))
  assert (got['match'] == href['match']).all()
  for k in names[:-1]:
    assert abs(float(got[k]) - float(href[k])) < 2e-4 * max(1.0, abs(float(href[k]))), k


def test_weights_reload_invalidates_packing(cuda):
  import full_model
  opt = ora.make_opt('cvppp', 64, 64, 2)
  x, _, _ = _inputs(opt, 1, 5)
  m = full_model.get_model(opt)
  for seed in (1, 2):
    P = ora.random_params(opt, seed)
    m.load_weights(P)
    y = m.run('y_out', {'x': x, 'phase_train': False}, as_numpy=True)
    ref = ora.full_model_forward(opt, P, x)
    assert np.abs(y - ref['y_out']).max() < MASK_TOL
  # the engine compares the weights' stamp AFTER it has launched (the host work hides behind the GPU) and launches again if it
  # changed: an in-place edit of one tensor between two forwards — graph captured, same buffers — must show in the second one
  key = 'ctrl_mlp_b_0'
  P = dict(P)
  b = np.array(P[key], copy=True)
  b[0:2] += 0.3
  P[key] = b
  with torch.no_grad():
    m[key].copy_(torch.as_tensor(b).to(m[key].device, m[key].dtype).reshape(m[key].shape))
  y = m.run('y_out', {'x': x, 'phase_train': False}, as_numpy=True)
  ref2 = ora.full_model_forward(opt, P, x)
  assert np.abs(y - ref2['y_out']).max() < MASK_TOL
  assert np.abs(ref2['y_out'] - ref['y_out']).max() > 10 * MASK_TOL  # (the edit does move the masks)


def test_box_model(cuda):
  import box_model
  opt = ora.make_opt('cvppp', 96, 96, 3)
  B = 2
  P = ora.random_params(opt, 7, box_model=True)
  rng = np.random.RandomState(8)
  x = rng.rand(B, 96, 96, 3).astype(np.float32)
  y_gt = np.zeros((B, 3, 96, 96), np.float32)
  y_gt[:, 0, 10:40, 15:50] = 1
  y_gt[:, 1, 50:80, 40:90] = 1
  noise = rng.uniform(0, 0.3, (3, B, 96, 96, 1)).astype(np.float32)
  ref = ora.box_model_forward(opt, P, x, y_gt, noise)
  m = box_model.get_model(opt).load_weights(P)
  names = ['s_out', 'attn_box', 'attn_ctr', 'attn_size', 'canvas']
  out = dict(zip(names, m.run(names, {'x': x, 'y_gt': y_gt, 'noise': noise[..., 0],
                                      'phase_train': False}, as_numpy=True)))
  for k in names:
    assert np.abs(out[k] - ref[k]).max() < (2e-3 if k.startswith('attn_c') or k == 'attn_size'
                                            else MASK_TOL), k


def test_operator_surface_closures(cuda):
  """The nnlib-shaped closures (cnn / dcnn / mlp / lstm) against the oracle, layer by layer."""
  import nnlib as nn
  import modellib
  rng = np.random.RandomState(3)
  model = {}
  run = nn.cnn([3, 3], [4, 8, 16], [1, 2], [nn.relu, nn.relu], [True, True], phase_train=False,
               scope='t_cnn', model=model)
  run.declare_copies(2)
  P = {}
  for k, v in model.items():
    a = rng.uniform(0.5, 1.5, tuple(v.shape)) if ('gamma' in k or 'var' in k) else \
        rng.randn(*v.shape) * 0.3
    v.copy_(torch.from_numpy(a.astype(np.float32)))
    P[k] = a.astype(np.float32).astype(np.float64)
  x = rng.randn(2, 16, 16, 4).astype(np.float32)
  xd = torch.from_numpy(x).to(cuda)
  for cp in range(2):
    h = run(xd)
    ref = ora.run_cnn(x.astype(np.float64), P, 't_cnn', 2, [1, 2], cp)
    for a, b in zip(h, ref):
      assert np.abs(a.cpu().numpy() - b).max() < 1e-4
  assert sorted(model) == sorted(['t_cnn_w_0', 't_cnn_b_0', 't_cnn_w_1', 't_cnn_b_1'] + [
      't_cnn_%d_%d_%s' % (i, c, n) for i in range(2) for c in range(2)
      for n in ('beta', 'gamma', 'ema_mean', 'ema_var')])
  # conv2d / max_pool / gaussian filter / extract_patch stand-alone operators
  w = rng.randn(3, 3, 4, 8).astype(np.float32)
  y = nn.conv2d(xd, torch.from_numpy(w).to(cuda)).cpu().numpy()
  assert np.abs(y - ora.conv2d(x.astype(np.float64), w.astype(np.float64))).max() < 1e-4
  assert (nn.max_pool(xd, 2).cpu().numpy() == ora.max_pool(x, 2)).all()
  cell = nn.lstm(8, 16, scope='t_lstm', model=model)
  PL = {k: model[k].cpu().numpy().astype(np.float64) for k in model if k.startswith('t_lstm')}
  inp, st = rng.randn(3, 8).astype(np.float32), rng.randn(3, 32).astype(np.float32)
  s2, gi, gf, go = cell(torch.from_numpy(inp).to(cuda), torch.from_numpy(st).to(cuda))
  r2, ri, rf, ro = ora.lstm_step(inp.astype(np.float64), st.astype(np.float64), PL, 't_lstm', 16)
  assert np.abs(s2.cpu().numpy() - r2).max() < 1e-5 and np.abs(go.cpu().numpy() - ro).max() < 1e-5
  f = modellib.get_gaussian_filter(torch.tensor([20.0, 30.0], device=cuda),
                                   torch.tensor([25.0, 40.0], device=cuda),
                                   torch.tensor([0.1, 0.5], device=cuda), 64, 48)
  fr = ora.get_gaussian_filter(np.array([20.0, 30.0]), np.array([25.0, 40.0]),
                               np.array([0.1, 0.5]), 64, 48)
  assert np.abs(f.cpu().numpy() - fr).max() < 1e-5


@pytest.mark.parametrize('name', ['full_model_cvppp_128', 'full_model_kitti_64x96'])
def test_golden_fixture(cuda, name):
  """The committed vectors (tests/golden/*.npz: seeded inputs -> oracle outputs)."""
  import os
  import full_model
  fx = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', name + '.npz'),
               allow_pickle=True)
  opt = fx['opt'].item()
  P = ora.random_params(opt, int(fx['seed']))
  feed = {'x': fx['x'], 'phase_train': False}
  for k in ('d_in', 'y_in'):
    if k in fx.files:
      feed[k] = fx[k]
  m = full_model.get_model(opt).load_weights(P)
  names = ['y_out', 's_out', 'attn_ctr', 'attn_size', 'x_patch', 'ctrl_rnn_glimpse_map']
  out = dict(zip(names, m.run(names, feed, as_numpy=True)))
  assert np.abs(out['y_out'] - fx['y_out']).max() < MASK_TOL
  assert np.abs(out['s_out'] - fx['s_out']).max() < MASK_TOL
  assert np.abs(out['x_patch'] - fx['x_patch']).max() < 1e-3
  assert np.abs(out['attn_ctr'] - fx['attn_ctr']).max() < 2e-3
  assert np.abs(out['ctrl_rnn_glimpse_map'] - fx['ctrl_rnn_glimpse_map']).max() < 1e-4


def test_full_size_properties(cuda):
  """BASELINE.json configs[1] shape (512x512, T=16, B=8): size-independent properties — canvas
  monotone = running max of the masks, masks in (0,1), glimpse maps sum to one, batch rows
  independent of their neighbours (same image alone == same image inside a batch)."""
  import bench
  import full_model
  opt = bench.make_opt('cvppp', 512, 512, 16)
  m = full_model.get_model(opt)
  bench.seed_weights(m, 3)
  g = torch.Generator().manual_seed(0)
  x = torch.rand((8, 512, 512, 3), generator=g)
  y, s, gm, cv = m.run(['y_out', 's_out', 'ctrl_rnn_glimpse_map', 'canvas'],
                       {'x': x, 'phase_train': False})
  assert y.shape == (8, 16, 512, 512) and s.shape == (8, 16)
  assert bool(((y > 0) & (y < 1)).all()) and bool(((s > 0) & (s < 1)).all())
  assert float((gm.sum(dim=(3, 4)) - 1).abs().max()) < 1e-5
  assert float((y.max(dim=1)[0] - cv[..., 0]).abs().max()) < 1e-6
  m.engine.nsub = 1
  y1 = m.run('y_out', {'x': x[2:3], 'phase_train': False})
  assert float((y1 - y[2:3]).abs().max()) < 1e-5


def test_cfg2_full_size_vs_oracle(cuda):
  """BASELINE.json configs[1] at FULL size — CVPPP arch, 512x512, T=16 — against the float64
  oracle with oracle-style weights (non-trivial masks), B=2; masks within 1e-3.  (Weights, images and the oracle's answer are those
  of the pipelined operating-point test below: at 512 px the seeded weights leave every mask at sigmoid(-5), so the box gets a
  plausible size and the decoder's last BN a positive offset; the float64 forward is computed once per session.)"""
  c = _cfg2_operating_point_case()
  out, ref = _check(c['opt'], 2, 101, use_graph=True, tune=lambda P: c['P'], ref=c['ref'])
  assert ref['y_out'].max() > 0.9 and (ref['y_out'] > 0.5).mean() > 0.01
  print('cfg2 full size: max |dy| = %.2e' % np.abs(out['y_out'] - ref['y_out']).max())


_CFG2_OP = {}


def _cfg2_operating_point_case():
  """cfg2 weights tuned to non-trivial masks + the float64 oracle on two images (computed once per session)."""
  if not _CFG2_OP:
    opt = ora.make_opt('cvppp', 512, 512, 16)
    P = dict(ora.random_params(opt, 101))
    b = P['ctrl_mlp_b_0'].copy()
    b[0:2], b[2:4] = [0.1, -0.2], np.log(0.3)
    P['ctrl_mlp_b_0'] = b
    for t in range(16):
      P['attn_dcnn_6_%d_beta' % t] = P['attn_dcnn_6_%d_beta' % t] + 12.0
    x2, _, _ = _inputs(opt, 2, 102)
    _CFG2_OP.update(opt=opt, P=P, x2=x2, ref=ora.full_model_forward(opt, P, x2, None, None))
  return _CFG2_OP


@pytest.mark.parametrize('depth,coalesce', [(4, 2), (8, 1)], ids=['bench_default_4_slots_of_2x8', 'one_batch_per_slot'])
def test_cfg2_pipelined_operating_point_vs_oracle(cuda, depth, coalesce):
  """The operating point bench.py times, built exactly as bench.py builds it (`model.pipeline(in_flight // coalesce,
  coalesce=coalesce)` with --in-flight 8, --coalesce 2: four slots on four streams, each decoding TWO consecutively submitted
  batches of 8 as ONE 16-image forward — K2b in groups of 8, every controller-CNN kernel at twice the tile count, the y_out
  prefill rider over 16 images) — cfg2 (512x512, T=16), eight batches of 8 submitted, against the float64 oracle: the oracle's
  two images sit at positions 2 and 5 of EVERY batch, so both halves of a slot's 16-image launch are checked.  The
  one-batch-per-slot case (rounds 2-4's protocol: K2b in groups of 4) stays beside it."""
  import full_model
  c = _cfg2_operating_point_case()
  ref = c['ref']
  rng = np.random.RandomState(7)
  feeds = []
  for k in range(2):  # two different batches alternate, so that a slot's two members differ in their other six images
    x8 = rng.rand(8, 512, 512, 3).astype(np.float32)
    x8[2], x8[5] = c['x2'][0], c['x2'][1]
    feeds.append({'x': torch.as_tensor(x8).cuda(), 'phase_train': False})
  m = full_model.get_model(c['opt']).load_weights(c['P'])
  pipe = m.pipeline(max(1, 8 // coalesce), coalesce=coalesce)  # bench.py: model.pipeline(in_flight // coalesce, coalesce=coalesce)
  assert pipe.streams == 4 and pipe.depth == depth
  for k in range(8):
    assert not pipe.full()
    pipe.submit(['y_out', 's_out'], feeds[k % 2])
  assert not pipe.free and not pipe.group  # every slot busy, nothing waiting for company
  outs = []
  while len(pipe):
    outs.append(pipe.collect(as_numpy=True))
  sb = pipe.slots[0][0].subs[0]
  assert sb.get('ctrl_batch')  # the slots run the group-shared controller
  assert int(sb['img'].shape[0]) == 8 * coalesce  # ... over the images of `coalesce` batches
  for k, (y, s) in enumerate(outs):
    y0, s0 = outs[k % 2]
    assert (y == y0).all() and (s == s0).all()  # the same batch in another slot / the other half of a launch: bit-identical
    for j, pos in enumerate((2, 5)):
      assert np.abs(y[pos] - ref['y_out'][j]).max() < MASK_TOL and np.abs(s[pos] - ref['s_out'][j]).max() < MASK_TOL
  assert ref['y_out'].max() > 0.9


def _bench_pipeline(m, stages, in_flight, coalesce, B):
  """The DecodePipeline bench.py --config cfg3|cfg5 builds for one stage (bench.bench_other: no --part-images, default streams)."""
  depth = max(1, in_flight // stages // coalesce)
  return m.pipeline(depth, max_images=B * coalesce, co_resident=min(depth, 4) * stages, streams=None, coalesce=coalesce)


def test_cfg3_coalesced_operating_point_vs_oracle(cuda):
  """bench.py --config cfg3 as it runs by default (--in-flight 8 --coalesce 2): KITTI arch 128x448, T = 20, both stages, every
  slot decoding TWO batches of 16 as one 32-image forward (more images than any multi-workgroup controller form takes at this
  co-residency: whatever form the engine picks is the one checked).  Four batches per stage; the oracle's two images sit at
  positions 3 and 12 of every batch — float64 oracle masks within 1e-3 for full_model, boxes and scores for box_model."""
  import box_model
  import full_model
  opt = ora.make_opt('kitti', 128, 448, 20)
  B, T, H, W = 16, 20, 128, 448
  x2, d2, y2 = _inputs(opt, 2, 62)
  rng = np.random.RandomState(11)
  xb, db, yb = _inputs(opt, B, 63)
  for k, pos in enumerate((3, 12)):
    xb[pos], db[pos], yb[pos] = x2[k], d2[k], y2[k]
  # stage 2: full_model
  P = ora.random_params(opt, 61)
  ref = ora.full_model_forward(opt, P, x2, d2, y2)
  m = full_model.get_model(opt).load_weights(P)
  pipe = _bench_pipeline(m, 2, 8, 2, B)
  assert pipe.depth == 2 and pipe.coalesce == 2
  feed = {'x': torch.as_tensor(xb).cuda(), 'd_in': torch.as_tensor(db).cuda(), 'y_in': torch.as_tensor(yb).cuda(), 'phase_train': False}
  for _ in range(4):
    assert not pipe.full(B)
    pipe.submit(['y_out', 's_out'], feed)
  outs = []
  while len(pipe):
    outs.append(pipe.collect(as_numpy=True))
  assert int(pipe.slots[0][0].subs[0]['img'].shape[0]) == 32
  for y, s in outs:
    for k, pos in enumerate((3, 12)):
      assert np.abs(y[pos] - ref['y_out'][k]).max() < MASK_TOL and np.abs(s[pos] - ref['s_out'][k]).max() < MASK_TOL
  print('cfg3 full_model slot controller:', 'K2b' if pipe.slots[0][0].subs[0].get('ctrl_batch') else
        'split' if 'ctrl_ws' in pipe.slots[0][0].subs[0] else 'one workgroup per image')
  del pipe, m
  # stage 1: box_model (teacher-forced canvas from y_gt and the fed noise)
  Pb = ora.random_params(opt, 64, box_model=True)
  y_gt2 = np.zeros((2, T, H, W), np.float32)
  for b in range(2):
    for t in range(3):
      y0, x0 = rng.randint(0, H // 2), rng.randint(0, W // 2)
      y_gt2[b, t, y0:y0 + rng.randint(8, H // 2), x0:x0 + rng.randint(8, W // 2)] = 1
  noise2 = rng.uniform(0, 0.3, (T, 2, H, W, 1)).astype(np.float32)
  refb = ora.box_model_forward(opt, Pb, x2, y_gt2, noise2, d_in=d2, y_in=y2)
  y_gtb = np.zeros((B, T, H, W), np.float32)
  y_gtb[:, 0, 10:60, 20:200] = 1
  noiseb = rng.uniform(0, 0.3, (T, B, H, W)).astype(np.float32)
  for k, pos in enumerate((3, 12)):
    y_gtb[pos], noiseb[:, pos] = y_gt2[k], noise2[:, k, :, :, 0]
  mb = box_model.get_model(opt).load_weights(Pb)
  pipe = _bench_pipeline(mb, 2, 8, 2, B)
  feedb = dict(feed, y_gt=torch.as_tensor(y_gtb).cuda(), noise=torch.as_tensor(noiseb).cuda())
  for _ in range(4):
    pipe.submit(['attn_box', 's_out'], feedb)
  while len(pipe):
    ab, sc = pipe.collect(as_numpy=True)
    for k, pos in enumerate((3, 12)):
      assert np.abs(ab[pos] - refb['attn_box'][k]).max() < MASK_TOL and np.abs(sc[pos] - refb['s_out'][k]).max() < MASK_TOL
  assert int(pipe.slots[0][0].subs[0]['img'].shape[0]) == 32


def test_cfg5_coalesced_operating_point_vs_oracle(cuda):
  """bench.py --config cfg5 as it runs by default (--in-flight 8 --coalesce 4): Cityscapes arch 256x512, T = 20, batches of 4,
  every slot decoding FOUR batches as one 16-image forward; the oracle's two images at positions 1 and 2 of every batch."""
  import full_model
  opt = ora.make_opt('cityscapes', 256, 512, 20)
  B = 4
  P = ora.random_params(opt, 71)
  x2, d2, y2 = _inputs(opt, 2, 72)
  ref = ora.full_model_forward(opt, P, x2, d2, y2)
  m = full_model.get_model(opt).load_weights(P)
  pipe = _bench_pipeline(m, 1, 8, 4, B)
  assert pipe.depth == 2 and pipe.coalesce == 4
  feeds = []
  for k in range(2):
    xb, db, yb = _inputs(opt, B, 73 + k)
    for j, pos in enumerate((1, 2)):
      xb[pos], db[pos], yb[pos] = x2[j], d2[j], y2[j]
    feeds.append({'x': torch.as_tensor(xb).cuda(), 'd_in': torch.as_tensor(db).cuda(), 'y_in': torch.as_tensor(yb).cuda(), 'phase_train': False})
  for k in range(8):
    assert not pipe.full(B)
    pipe.submit(['y_out', 's_out'], feeds[k % 2])
  assert not pipe.free
  n = 0
  while len(pipe):
    y, s = pipe.collect(as_numpy=True)
    n += 1
    for j, pos in enumerate((1, 2)):
      assert np.abs(y[pos] - ref['y_out'][j]).max() < MASK_TOL and np.abs(s[pos] - ref['s_out'][j]).max() < MASK_TOL
  assert n == 8 and int(pipe.slots[0][0].subs[0]['img'].shape[0]) == 16


def test_cfg5_cityscapes_t32(cuda):
  """The cfg5 T=32 variant on the Cityscapes arch (9 semantic classes, skips, dynamic_var)."""
  _check(ora.make_opt('cityscapes', 64, 128, 32), 1, 111, use_graph=True)


def _box_case(arch, H, W, T, B, seed, **over):
  import box_model
  opt = ora.make_opt(arch, H, W, T, **over)
  P = ora.random_params(opt, seed, box_model=True)
  rng = np.random.RandomState(seed + 1)
  x, d_in, y_in = _inputs(opt, B, seed + 2)
  y_gt = np.zeros((B, T, H, W), np.float32)
  for b in range(B):
    for t in range(min(T, 3)):
      y0, x0 = rng.randint(0, H // 2), rng.randint(0, W // 2)
      y_gt[b, t, y0:y0 + rng.randint(8, H // 2), x0:x0 + rng.randint(8, W // 2)] = 1
  noise = rng.uniform(0, 0.3, (T, B, H, W, 1)).astype(np.float32)
  ref = ora.box_model_forward(opt, P, x, y_gt, noise, d_in=d_in, y_in=y_in)
  m = box_model.get_model(opt).load_weights(P)
  names = ['s_out', 'attn_box', 'attn_ctr', 'attn_size', 'canvas']
  feed = {'x': x, 'y_gt': y_gt, 'noise': noise[..., 0], 'phase_train': False, 'd_in': d_in, 'y_in': y_in}
  for rep in range(2):  # second pass = HIP-graph replay
    out = dict(zip(names, m.run(names, feed, as_numpy=True)))
    for k in names:
      assert out[k].shape == ref[k].shape, k
      assert np.abs(out[k] - ref[k]).max() < (2e-3 if k.startswith('attn_c') or k == 'attn_size'
                                              else MASK_TOL), k
  return out, ref


def test_box_model_kitti_native_size(cuda):
  """cfg3's first stage on its own arch: box_model, KITTI arch at 128x448 with d_in / y_in (13
  input channels packed to 16), fixed_var default True (box_model.py:58-61)."""
  _box_case('kitti', 128, 448, 4, 2, 121)


def test_box_model_softmax_score(cuda):
  """num_semantic_classes > 1: the score is a softmax over classes (box_model.py:508-513)."""
  out, ref = _box_case('cityscapes', 64, 128, 3, 2, 131)
  assert out['s_out'].shape == (2, 3, 9) and abs(float(out['s_out'][0, 0].sum()) - 1.0) < 1e-5


def test_starved_split_controller_recovers_on_one_workgroup_form(cuda):
  """the 16-workgroup controller relies on all its workgroups being resident; a launch that is not (another
  process on the GPU) times out and flags its status word.  model.run and the pipeline's collect() then decode the same
  inputs again on the one-workgroup controller (no cross-workgroup waits) instead of raising or returning garbage, and the
  engine keeps that form.  Simulated by flagging the status word after a healthy forward."""
  import warnings
  import full_model
  opt = ora.make_opt('cvppp', 128, 128, 3)
  P = ora.random_params(opt, 43)
  m = full_model.get_model(opt).load_weights(P)
  x = np.random.RandomState(6).rand(2, 128, 128, 3).astype(np.float32)
  good = m.run(['y_out', 's_out'], {'x': x, 'phase_train': False}, as_numpy=True)
  eng = m.engine
  assert 'ctrl_ws' in eng.subs[0]  # the split form ran
  eng.subs[0]['y_out'].fill_(7.0)  # "garbage"
  eng.subs[0]['ctrl_status'].fill_(1)
  with warnings.catch_warnings(record=True) as w:
    warnings.simplefilter('always')
    assert eng.check_status() is True
  assert any('one-workgroup controller' in str(x_.message) for x_ in w)
  assert 'ctrl_ws' not in eng.subs[0] and eng.ctrl_split is False
  y2, s2 = eng.fetch('y_out').cpu().numpy(), eng.fetch('s_out').cpu().numpy()
  assert np.abs(y2 - good[0]).max() < 1e-4 and np.abs(s2 - good[1]).max() < 1e-4  # another summation order, the same masks
  again = m.run(['y_out', 's_out'], {'x': x, 'phase_train': False}, as_numpy=True)  # and it stays on that form
  assert np.array_equal(again[0], y2) and eng.check_status() is False
  with pytest.raises(Exception):
    eng.subs[0]['ctrl_status'] = torch.ones(1, dtype=torch.int32, device=cuda)
    eng.check_status(recover=False)
  # the pipeline's to_host path: the pinned host copies are taken inside submit(), from the starved forward;
  # collect() must hand back the RE-DECODED outputs, not those copies
  m2 = full_model.get_model(opt).load_weights(P)
  pipe = m2.pipeline(1)
  pipe.submit(['y_out', 's_out'], {'x': torch.as_tensor(x).cuda(), 'phase_train': False}, to_host=True)
  torch.cuda.synchronize()
  e2 = pipe.slots[0][0]
  assert 'ctrl_ws' in e2.subs[0]
  events = pipe.pending[0]['launch']['events']
  events[0][1][0].fill_(7.0)  # what a starved forward would have left in the pinned buffer
  e2.subs[0]['ctrl_status'].fill_(1)
  with warnings.catch_warnings(record=True):
    warnings.simplefilter('always')
    y3, s3 = pipe.collect()
  assert isinstance(y3, np.ndarray) and np.abs(y3 - good[0]).max() < 1e-4 and np.abs(s3 - good[1]).max() < 1e-4


def test_xcd_local_controller_with_part_of_its_xcd_taken(cuda):
  """The XCD-local controller (ra_ctrl_split.hip, XL form: the 16 workgroups of image b run on XCD b % 8 and exchange through
  that XCD's L2; roles are per-XCD tickets) under a REAL uneven deal instead of a simulated status word: a parked kernel
  (ra_debug_park_xcd) holds 24 of XCD 0's 32 CUs — 100 KB of LDS each, so none of them can take a 112 KB controller workgroup —
  for longer than the controller's spin limit.  Image 0's team then cannot be resident together: whether the dispatcher holds
  its other workgroups back (the residents time out on their peers) or deals them to other XCDs (tickets beyond an XCD's share
  wrap onto roles that exist; XCD 0's team stays short), the launch must flag its status word, model.run must decode the batch
  again on the one-workgroup controller, and the masks must be the oracle's.
  The parked kernel runs in a child process: the HIP runtime multiplexes a process's streams onto a few hardware queues
  (GPU_MAX_HW_QUEUES), so a side stream of this process can share a queue with the stream that polls the parked count or
  with the run's own streams, and everything queued behind the park then starts only after it has ended.  A second process
  has hardware queues of its own; in it, the park goes on a high-priority stream (its own queue pool) and the poll on the
  null stream."""
  import os
  import select
  import subprocess
  import sys
  import time
  import warnings
  import full_model
  opt = ora.make_opt('cvppp', 128, 128, 2)
  P = ora.random_params(opt, 47)
  x = np.random.RandomState(12).rand(2, 128, 128, 3).astype(np.float32)
  ref = ora.full_model_forward(opt, P, x, None, None)
  m = full_model.get_model(opt).load_weights(P)
  feed = {'x': x, 'phase_train': False}
  good = m.run(['y_out', 's_out'], feed, as_numpy=True)
  eng = m.engine
  sb = eng.subs[0]
  if 'ctrl_ws' not in sb or sb.get('ctrl_batch'):
    pytest.skip('the per-image split controller is not what this engine runs')
  assert np.abs(good[0] - ref['y_out']).max() < MASK_TOL
  torch.cuda.synchronize()
  park = ('import sys, time\n'
          'sys.path.insert(0, %r)\n'
          'import torch\n'
          'import ra_ops as ops\n'
          'resident = torch.zeros(1, dtype=torch.int32, device="cuda")\n'
          'side = torch.cuda.Stream(priority=-1)\n'
          'torch.cuda.synchronize()\n'
          'ops.park_xcd(0, 24, lds_bytes=100 * 1024, millis=12000, resident=resident, stream=side)\n'
          't0 = time.time()\n'
          'while int(resident.item()) < 24 and time.time() - t0 < 5.0:\n'
          '  time.sleep(0.01)\n'
          'print("parked %%d %%.3f" %% (int(resident.item()), time.time() - t0), flush=True)\n'
          'torch.cuda.synchronize()\n' % os.path.dirname(os.path.abspath(full_model.__file__)))
  child = subprocess.Popen([sys.executable, '-c', park], stdout=subprocess.PIPE, text=True)
  try:
    line = ''
    t0 = time.time()
    while not line.startswith('parked') and time.time() - t0 < 120.0:
      if select.select([child.stdout], [], [], 120.0 - (time.time() - t0))[0]:
        line = child.stdout.readline()
        if not line:
          break  # the child ended without reporting
    assert line.startswith('parked'), 'the parking process did not report (exit status %s)' % child.poll()
    n_parked, t_park = int(line.split()[1]), float(line.split()[2])
    assert n_parked == 24 and t_park < 5.0, 'parked workgroups resident on XCD 0: %d after %.2f s' % (n_parked, t_park)
    with warnings.catch_warnings(record=True) as w:
      warnings.simplefilter('always')
      t0 = time.time()
      y, s = m.run(['y_out', 's_out'], feed, as_numpy=True)
      dt = time.time() - t0
    torch.cuda.synchronize()
    still_parked = child.poll() is None
  finally:
    try:
      child.wait(timeout=60)
    except subprocess.TimeoutExpired:
      child.kill()
      child.wait()
  assert child.returncode == 0, 'parking process exit status %d' % child.returncode
  timed_out = any('one-workgroup controller' in str(x_.message) for x_ in w)
  print('run with 24 CUs of XCD 0 parked: %.2f s (park still running at its end: %s), timed out and re-decoded: %s'
        % (dt, still_parked, timed_out))
  # 8 free CUs on XCD 0 < 16 workgroups: the team could not have been resident together
  assert timed_out and eng.ctrl_split is False and 'ctrl_ws' not in eng.subs[0]
  assert np.abs(y - ref['y_out']).max() < MASK_TOL and np.abs(s - ref['s_out']).max() < MASK_TOL
  assert np.abs(y - good[0]).max() < 1e-4
  # the engine stays on the one-workgroup form and stays right
  y2 = m.run('y_out', feed, as_numpy=True)
  assert np.array_equal(y2, y)


def test_decode_pipeline_coalesced_batches_match_lone_runs(cuda, monkeypatch):
  """DecodePipeline(coalesce=2) (round 5): two consecutively submitted batches are decoded by ONE slot as one forward over
  their images, and collect() still returns them one at a time — each exactly what a lone model.run of that batch returns
  (eval-mode images are independent).  Ragged batch sizes, an odd batch count (the last one is launched alone by collect()),
  to_host, a change of the requested outputs inside a group, and parts (max_images) under coalescing."""
  import full_model
  opt = ora.make_opt('cvppp', 128, 160, 4)
  P = ora.random_params(opt, 44)
  m = full_model.get_model(opt).load_weights(P)
  rng = np.random.RandomState(8)
  sizes = [3, 2, 3, 3, 1, 3, 2]
  feeds = [{'x': rng.rand(b, 128, 160, 3).astype(np.float32), 'phase_train': False} for b in sizes]
  names = ['y_out', 's_out', 'x_patch']
  lone = [m.run(names, f, as_numpy=True) for f in feeds]
  for kw in (dict(), dict(to_host=True)):
    pipe = m.pipeline(2, coalesce=2)
    got = []
    for f in feeds:
      while pipe.full(f['x'].shape[0]):
        got.append(pipe.collect(as_numpy=True))
      pipe.submit(names, f, **kw)
    assert len(pipe) == len(feeds) - len(got)
    while len(pipe):
      got.append(pipe.collect(as_numpy=True))
    assert len(got) == len(lone) and sorted(pipe.free) == [0, 1] and not pipe.group
    for a, b in zip(got, lone):
      for u, v in zip(a, b):
        assert u.shape == v.shape and np.abs(u - v).max() < 1e-6, np.abs(u - v).max()
  # device tensors come back as copies: the slot's buffers are rewritten by its next launch
  pipe = m.pipeline(1, coalesce=2)
  pipe.submit('y_out', feeds[0])
  pipe.submit('y_out', feeds[1])
  y0 = pipe.collect()
  y1 = pipe.collect()
  pipe.submit('y_out', feeds[2])
  pipe.submit('y_out', feeds[3])
  pipe.drain()
  assert np.abs(y0.cpu().numpy() - lone[0][0]).max() < 1e-6 and np.abs(y1.cpu().numpy() - lone[1][0]).max() < 1e-6
  # another set of outputs closes the waiting group instead of joining it
  pipe = m.pipeline(2, coalesce=2)
  pipe.submit('y_out', feeds[0])
  pipe.submit(['s_out'], feeds[1])
  assert len(pipe.free) == 1 and len(pipe.group) == 1
  a = pipe.collect(as_numpy=True)
  b = pipe.collect(as_numpy=True)
  assert np.abs(a - lone[0][0]).max() < 1e-6 and np.abs(b[0] - lone[1][1]).max() < 1e-6
  # the end of a finite stream (round 6): with `remaining` told, the last batches stop waiting for company once what is left fits
  # the slots one batch each — 7 batches through 2 slots of 2: (0,1) (2,3) (4,5) then 6 alone as soon as a slot is free — and a
  # slot switches between its 2-batch and 1-batch sizes without losing either's buffers or graphs
  monkeypatch.setenv('RA_PIPE_ENDGAME', '1')  # (opt-in: measured slower at cfg2)
  pipe = m.pipeline(2, coalesce=2)
  got, launched_alone = [], 0
  for k, f in enumerate(feeds):
    left = len(feeds) - 1 - k
    while pipe.full(f['x'].shape[0], remaining=left):
      got.append(pipe.collect(as_numpy=True))
    before = len(pipe.group)
    pipe.submit(names, f, remaining=left)
    launched_alone += int(before == 0 and not pipe.group and left + 1 <= pipe.depth)
  while len(pipe):
    got.append(pipe.collect(as_numpy=True))
  assert launched_alone >= 1 and len(got) == len(lone)
  for a, b in zip(got, lone):
    for u, v in zip(a, b):
      assert u.shape == v.shape and np.abs(u - v).max() < 1e-6
  for f, l in zip(feeds[:2], lone[:2]):  # the same pipeline again: sizes it has seen come back from the engines' parked states
    pipe.submit(names, f, remaining=None)
  for l in lone[:2]:
    for u, v in zip(pipe.collect(as_numpy=True), l):
      assert np.abs(u - v).max() < 1e-6
  monkeypatch.setenv('RA_PIPE_ENDGAME', '0')
  # parts under coalescing: 3 + 3 images as three launches of 2
  pipe = m.pipeline(3, max_images=2, coalesce=2)
  pipe.submit(names, feeds[2])
  pipe.submit(names, feeds[3])
  assert len(pipe.free) == 0
  for k in (2, 3):
    r = pipe.collect(as_numpy=True)
    for u, v in zip(r, lone[k]):
      assert u.shape == v.shape and np.abs(u - v).max() < 1e-6
  assert sorted(pipe.free) == [0, 1, 2]


def test_decode_pipeline_matches_lone_run(cuda):
  """Batches in flight on their own HIP streams (full_model.DecodePipeline, the evaluator's loop)
  return, batch for batch, exactly what a lone model.run returns — including a ragged last
  batch and two laps over the slots — and the oracle's masks."""
  import full_model
  from ra_native import RecAttendError
  opt = ora.make_opt('cvppp', 128, 160, 6)
  P = ora.random_params(opt, 41)
  m = full_model.get_model(opt).load_weights(P)
  rng = np.random.RandomState(5)
  sizes = [3, 3, 3, 3, 3, 3, 3, 2]
  feeds = [{'x': rng.rand(b, 128, 160, 3).astype(np.float32), 'phase_train': False} for b in sizes]
  names = ['y_out', 's_out', 'attn_box', 'x_patch']
  lone = [m.run(names, f, as_numpy=True) for f in feeds]
  pipe = m.pipeline(3)
  got = []
  for f in feeds:
    if pipe.full():
      got.append(pipe.collect(as_numpy=True))
    pipe.submit(names, f)
  with pytest.raises(KeyError):
    pipe.submit(['loss'], feeds[0])
  while len(pipe):
    got.append(pipe.collect(as_numpy=True))
  with pytest.raises(RecAttendError):
    pipe.collect()
  assert len(got) == len(lone)
  for a, b in zip(got, lone):
    for u, v in zip(a, b):
      assert u.shape == v.shape and np.array_equal(u, v)
  ref = ora.full_model_forward(opt, P, feeds[-1]['x'], None, None)
  assert np.abs(got[-1][0] - ref['y_out']).max() < MASK_TOL
  # full pipeline refuses a further submit instead of overwriting a batch not yet collected
  for f in feeds[:3]:
    pipe.submit('y_out', f)
  with pytest.raises(RecAttendError):
    pipe.submit('y_out', feeds[0])
  assert np.array_equal(pipe.collect(as_numpy=True), lone[0][0])
  pipe.drain()
  assert len(pipe) == 0
  # a batch cut into parts of <= 2 images (3 slots for 5 images) comes back whole and in order
  x5 = rng.rand(5, 128, 160, 3).astype(np.float32)
  whole = m.run(names, {'x': x5, 'phase_train': False}, as_numpy=True)
  cut = m.pipeline(3, max_images=2)
  assert cut.parts(5) == 3 and not cut.full(5)
  cut.submit(names, {'x': x5, 'phase_train': False})
  assert cut.full() and cut.full(5)
  with pytest.raises(RecAttendError):
    cut.submit(names, {'x': x5, 'phase_train': False})
  for u, v in zip(cut.collect(as_numpy=True), whole):
    assert u.shape == v.shape and np.array_equal(u, v)
  with pytest.raises(RecAttendError):
    m.pipeline(2, max_images=2).submit(names, {'x': x5, 'phase_train': False})


def test_decode_pipeline_box_model(cuda):
  """box_model through the pipeline (y_gt and the canvas noise are cut with the batch)."""
  import box_model
  opt = ora.make_opt('kitti', 64, 96, 4)
  m = box_model.get_model(opt).load_weights(ora.random_params(opt, 3, box_model=True))
  rng = np.random.RandomState(2)
  B, T, H, W = 4, 4, 64, 96
  x, d_in, y_in = _inputs(opt, B, 7)
  y_gt = np.zeros((B, T, H, W), np.float32)
  y_gt[:, 0, 10:30, 20:50] = 1.0
  y_gt[:, 1, 35:60, 40:90] = 1.0
  noise = rng.uniform(0, 0.3, (T, B, H, W)).astype(np.float32)
  feed = {'x': x, 'd_in': d_in, 'y_in': y_in, 'y_gt': y_gt, 'noise': noise, 'phase_train': False}
  names = ['attn_box', 's_out']
  whole = m.run(names, feed, as_numpy=True)
  pipe = m.pipeline(2, max_images=2)
  pipe.submit(names, feed)
  for u, v in zip(pipe.collect(as_numpy=True), whole):
    assert u.shape == v.shape and np.array_equal(u, v)


def test_decode_pipeline_controller_policy(cuda):
  """Slots decode with the per-image 16-workgroup controller only if every launch that can run at the same
  time fits the chip (streams x images x 16 <= 224); otherwise with the group-shared form (K2b: 16 workgroups
  per group of images, resident many times over), whose results equal the per-image form's to round-off; and
  with the one-workgroup form where neither fits."""
  import full_model
  opt = ora.make_opt('cvppp', 64, 64, 3)
  P = ora.random_params(opt, 9)
  x = np.random.RandomState(3).rand(8, 64, 64, 3).astype(np.float32)
  feed = {'x': x, 'phase_train': False}
  m = full_model.get_model(opt).load_weights(P)
  split = m.run(['y_out', 's_out'], feed, as_numpy=True)
  assert 'ctrl_ws' in m.engine.subs[0] and not m.engine.subs[0].get('ctrl_batch')
  pipe = m.pipeline(4)  # 4 x 8 x 16 = 512 workgroups > 224; 4 x ceil(8 / group) x 16 <= 128 in the group-shared form
  pipe.submit(['y_out', 's_out'], feed)
  got = pipe.collect(as_numpy=True)
  assert pipe.slots[0][0].subs[0].get('ctrl_batch')
  for u, w in zip(got, split):
    assert np.abs(u - w).max() < 1e-4
  wide = m.pipeline(16, streams=16)  # 16 launches at a time x 16 workgroups or more > 224: the one-workgroup form
  wide.submit(['y_out', 's_out'], feed)
  got1 = wide.collect(as_numpy=True)
  assert 'ctrl_ws' not in wide.slots[0][0].subs[0]
  m2 = full_model.get_model(opt).load_weights(P)
  m2.engine.ctrl_split = False
  single = m2.run(['y_out', 's_out'], feed, as_numpy=True)
  for u, v, w in zip(got1, single, split):
    assert np.array_equal(u, v)
    assert np.abs(u - w).max() < 1e-4
  small = m.pipeline(1)  # 1 x 8 x 16 = 128
  small.submit('y_out', feed)
  assert np.array_equal(small.collect(as_numpy=True), split[0])
  assert 'ctrl_ws' in small.slots[0][0].subs[0] and not small.slots[0][0].subs[0].get('ctrl_batch')


def test_decode_pipeline_to_host(cuda):
  """submit(to_host=True): outputs arrive as NumPy arrays in pinned host memory, equal to model.run's."""
  import full_model
  opt = ora.make_opt('cvppp', 64, 64, 3)
  m = full_model.get_model(opt).load_weights(ora.random_params(opt, 2))
  rng = np.random.RandomState(8)
  feeds = [{'x': rng.rand(2, 64, 64, 3).astype(np.float32), 'phase_train': False} for _ in range(3)]
  lone = [m.run(['y_out', 's_out'], f, as_numpy=True) for f in feeds]
  pipe = m.pipeline(2)
  got = []
  for f in feeds:
    if pipe.full():
      got.append(pipe.collect())
    pipe.submit(['y_out', 's_out'], f, to_host=True)
  while len(pipe):
    got.append(pipe.collect())
  for a, b in zip(got, lone):
    for u, v in zip(a, b):
      assert isinstance(u, np.ndarray) and np.array_equal(u, v)


def test_decode_pipeline_coalesces_box_model_batches_and_drains_a_waiting_group(cuda):
  """box_model batches (y_gt and the [T, B, H, W] noise are fed per batch) through DecodePipeline(coalesce=2): each batch as a
  lone run; and drain() with every slot busy AND a batch still waiting for company (it used to raise: the waiting batch needs a
  slot that only the older, launched batches can give back)."""
  import box_model
  opt = ora.make_opt('cvppp', 96, 96, 3)
  P = ora.random_params(opt, 7, box_model=True)
  m = box_model.get_model(opt).load_weights(P)
  rng = np.random.RandomState(9)
  feeds = []
  for b in (2, 3, 2, 1, 2):
    y_gt = np.zeros((b, 3, 96, 96), np.float32)
    y_gt[:, 0, 10:40, 15:50] = 1
    y_gt[:, 1, 50:80, 40:90] = 1
    feeds.append({'x': rng.rand(b, 96, 96, 3).astype(np.float32), 'y_gt': y_gt,
                  'noise': rng.uniform(0, 0.3, (3, b, 96, 96)).astype(np.float32), 'phase_train': False})
  names = ['s_out', 'attn_box', 'canvas']
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
      assert u.shape == v.shape and np.abs(u - v).max() < 1e-6, np.abs(u - v).max()
  # two slots busy with two batches each, a fifth batch waiting for company: drain() must not raise
  pipe = m.pipeline(2, coalesce=2)
  for f in feeds:
    pipe.submit(names, f)
  assert len(pipe.group) == 1 and not pipe.free
  pipe.drain()
  assert not pipe.group and not len(pipe) and sorted(pipe.free) == [0, 1]
