"""The render stage on the device against tests/render_oracle.py.  The images are integers: equality, no tolerance — except
the orientation image's arg-max, which is float32 on the device and float64 in the oracle and is compared outside the 1e-5 gap
band of tests/test_pixel_eval_gpu.py, with the share of pixels inside the band capped as there."""
import functools
import os

import numpy as np
import pytest
import torch

import analysis
import cs_oracle as cso
import ra_native as rn
import ra_ops as ops
import render_oracle as ro
from utils import png

pytestmark = pytest.mark.gpu
GAP = 1e-5          # tests/test_pixel_eval_gpu.py
BAND_SHARE = 1e-3
# (B, T, H, W): 16-byte loads and dword stores; H * W % 4 != 0: element loads and byte stores; T beyond the 22 colours
INSTANCE_SHAPES = [(2, 3, 8, 12), (1, 1, 5, 7), (2, 23, 9, 10)]
# (Hs, Ws, H, W): an integer ratio, odd sizes with H * W % 4 != 0, and equal sizes
ORI_SHAPES = [(6, 10, 24, 40), (7, 9, 19, 31), (12, 14, 12, 14)]


def _dev(a, dtype=np.float32):
  return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


@functools.lru_cache(maxsize=None)
def _instances(shape):
  """One-label disc masks, plus an overlap and a value of 2.0 where there is room; per-image colour tables that differ."""
  B, T, H, W = shape
  rng = np.random.RandomState(B * 1000 + T * 100 + H)
  y = cso.disc_instances(rng, B, T, H, W, soft=False, rmin=0.15, rmax=0.45).astype(np.float32)
  if T >= 2:
    y[0, 1, : H // 2] = np.maximum(y[0, 1, : H // 2], y[0, 0, : H // 2])  # plane 1 overlaps plane 0
    y[-1, T - 1, H // 2:, : W // 2] = 2.0                                     # a value of 2.0, on top of what is there
  else:
    y[0, 0, 0, :3] = 2.0
  y[0, 0, H - 1, W - 1] = 0.7  # a soft value: draws nothing
  cols = rng.randint(0, 256, (B, T, 3)).astype(np.uint8)
  cols[:, 0, 1] = 0  # a zero channel in the first colour: FIRST lets a later plane fill it
  return y, cols


@pytest.mark.parametrize('shape', INSTANCE_SHAPES, ids=lambda s: '%dx%dx%dx%d' % s)
def test_render_instances_equals_the_oracle(cuda, shape):
  B, T, H, W = shape
  y, cols = _instances(shape)
  yd = _dev(y)
  got = ops.render_instances(yd)
  assert got.dtype == torch.uint8 and tuple(got.shape) == (B, H, W, 3) and got.is_contiguous()
  want = ro.render_instances(y)  # the default palette, CMAP[t % 22]
  assert want.any() and (got.cpu().numpy() == want).all()
  # per-image colour tables, both modes; the wrapper takes the image's B, G, R order, the oracle the reference's rows
  bgr = torch.from_numpy(np.ascontiguousarray(cols[:, :, ::-1])).cuda()
  add = np.stack([ro.add_image(y[b], cols[b])[:, :, ::-1] for b in range(B)]).astype(np.uint8)
  first = np.stack([ro.first_image(y[b], cols[b])[:, :, ::-1] for b in range(B)]).astype(np.uint8)
  assert (ops.render_instances(yd, colours=bgr).cpu().numpy() == add).all()
  assert (ops.render_instances(yd, colours=bgr, first=True).cpu().numpy() == first).all()
  if T >= 2:
    assert (add != first).any()  # the overlap tells the modes apart
  # one [T,3] table for every image
  one = np.stack([ro.first_image(y[b], cols[0])[:, :, ::-1] for b in range(B)]).astype(np.uint8)
  assert (ops.render_instances(yd, colours=bgr[0].contiguous(), first=True).cpu().numpy() == one).all()
  # nothing to draw: an all-zero image
  assert not ops.render_instances(torch.zeros_like(yd)).any() and not ops.render_instances(torch.zeros_like(yd), first=True).any()


def test_render_instances_unaligned_view(cuda):
  """y as a view that starts one element into its buffer: 4-byte aligned only, so the element path, with H * W % 4 == 0."""
  shape = INSTANCE_SHAPES[0]
  y, cols = _instances(shape)
  buf = torch.zeros(y.size + 1, dtype=torch.float32, device='cuda')
  view = buf[1:].view(*shape)
  view.copy_(_dev(y))
  assert view.data_ptr() % 16 == 4 and view.is_contiguous()
  bgr = torch.from_numpy(np.ascontiguousarray(cols[:, :, ::-1])).cuda()
  assert (ops.render_instances(view).cpu().numpy() == ro.render_instances(y)).all()
  first = np.stack([ro.first_image(y[b], cols[b])[:, :, ::-1] for b in range(shape[0])]).astype(np.uint8)
  assert (ops.render_instances(view, colours=bgr, first=True).cpu().numpy() == first).all()


def test_render_instances_refusals(cuda):
  y = torch.zeros(1, 2, 4, 4, device='cuda')
  with pytest.raises(rn.RecAttendError, match='colours'):
    ops.render_instances(y, colours=torch.zeros(3, 3, dtype=torch.uint8, device='cuda'))
  with pytest.raises(rn.RecAttendError):
    ops.render_instances(y, colours=torch.zeros(2, 3, device='cuda'))  # not uint8
  with pytest.raises(rn.RecAttendError):
    ops.render_instances(y[0])
  with pytest.raises(rn.RecAttendError, match='wheel'):
    ops.render_orientation(torch.zeros(1, 2, 2, 9, device='cuda'), torch.zeros(1, 4, 4, device='cuda'))
  with pytest.raises(rn.RecAttendError, match='size'):
    ops.render_orientation(torch.zeros(1, 2, 2, 8, device='cuda'), torch.zeros(1, 4, 4, device='cuda'), size=(4, 5))


@functools.lru_cache(maxsize=None)
def _ori_case(shape):
  """Seeded softmax maps d float32 [2,Hs,Ws,8], a mask with both values in every row, the float64 full-size planes, the
  oracle's image and the outside-the-band mask."""
  Hs, Ws, H, W = shape
  rng = np.random.RandomState(40 + Hs)
  lg = 2.0 * rng.randn(2, Hs, Ws, 8)
  d = (np.exp(lg) / np.exp(lg).sum(-1, keepdims=True)).astype(np.float32)
  mask = (rng.rand(2, H, W) > 0.3).astype(np.float32)
  mask[:, :, 0], mask[:, :, -1] = 1.0, 0.0
  full = ro.orientation_full(d, H, W)
  return d, mask, full, ro.orientation_image(full, mask), ro.orientation_gap(full) >= GAP


def test_orientation_oracle_inputs_stay_under_the_cap():
  """Needs no device, but belongs to the cases below: the seeded inputs leave at most BAND_SHARE of the pixels in the band and
  show all eight classes where the mask is 1."""
  for shape in ORI_SHAPES:
    d, mask, full, want, sure = _ori_case(shape)
    assert 1.0 - sure.mean() <= BAND_SHARE, shape
    assert sorted(np.unique(np.argmax(full, -1)[mask > 0])) == list(range(8)), shape
    assert all(((m == 0).any() and (m == 1).any()) for img in mask for m in img)


@pytest.mark.parametrize('shape', ORI_SHAPES, ids=lambda s: '%dx%d-%dx%d' % s)
def test_render_orientation_equals_the_float64_argmax_outside_the_band(cuda, shape):
  Hs, Ws, H, W = shape
  d, mask, full, want, sure = _ori_case(shape)
  share = 1.0 - sure.mean()
  print('pixels inside the band: %d of %d (%.5f %%)' % ((~sure).sum(), sure.size, 100 * share))
  assert share <= BAND_SHARE
  colours = {tuple(c) for c in want.reshape(-1, 3)}
  assert colours == {tuple(int(v) for v in row) for row in ro.WHEEL} | {(0, 0, 0)}  # all eight classes and the masked pixels
  got = ops.render_orientation(_dev(d), _dev(mask), size=(H, W))
  assert got.dtype == torch.uint8 and tuple(got.shape) == (2, H, W, 3)
  got = got.cpu().numpy()
  diff = (got != want).any(axis=-1)
  print('pixels that differ outside the band: %d; inside: %d' % (diff[sure].sum(), diff[~sure].sum()))
  assert not diff[sure].any()
  assert not got[mask == 0].any()


def test_render_orientation_ties_go_to_the_lower_channel(cuda):
  rng = np.random.RandomState(8)
  d = rng.rand(2, 6, 10, 8).astype(np.float32) * 0.5
  d[0, ..., 2] = d[0, ..., 5] = d[0].max(axis=-1) + rng.rand(6, 10).astype(np.float32)  # equal at every tap
  d[1, ..., 0] = d[1, ..., 7] = d[1].max(axis=-1) + rng.rand(6, 10).astype(np.float32)
  for H, W in ((24, 40), (19, 31), (6, 10)):
    mask = (rng.rand(2, H, W) > 0.4).astype(np.float32)
    got = ops.render_orientation(_dev(d), _dev(mask)).cpu().numpy()
    for b, cls in ((0, 2), (1, 0)):
      assert (got[b][mask[b] == 1] == ro.WHEEL[cls]).all() and not got[b][mask[b] == 0].any()


def test_analyzers_write_the_oracles_images(cuda, tmp_path):
  """The three render analyzers and the count file into a temporary folder: the decoded files equal the oracle's images."""
  names = ['a_000_x.png', 'b_111_y']
  files = lambda folder: [str(tmp_path / folder / 'b_111_y.png'), str(tmp_path / folder / 'a_000_x.png')]  # indices [1, 0]
  for shape in INSTANCE_SHAPES:
    y, _ = _instances(shape)
    folder = 'ins%d' % shape[1]
    r = analysis.RenderInstanceAnalyzer(str(tmp_path / folder), names)
    r.stage({'y_out': _dev(y), 'indices': [1, 0][:shape[0]]})
    want = ro.render_instances(y)
    assert r.written == files(folder)[:shape[0]]
    for b, f in enumerate(r.written):
      assert (png.read_colour8(f) == want[b]).all()
  # the count file and the ground-truth image count pixels with ops.pair_stats, which takes H * W % 4 == 0: 22 outputs of 8 x 10
  B, T, H, W = 2, 22, 8, 10
  rng = np.random.RandomState(5)
  y = cso.disc_instances(rng, B, T, H, W, soft=False, rmin=0.15, rmax=0.45).astype(np.float32)
  y_gt = cso.disc_instances(rng, B, 4, H, W, soft=False, rmin=0.2, rmax=0.5).astype(np.float32)
  y_gt[:, 2] = 0.0  # an empty ground-truth plane in the middle
  s_gt = np.array([[1, 1, 0, 1]] * B, np.float32)
  res = {'y_out': _dev(y), 'y_gt': _dev(y_gt), 's_gt': _dev(s_gt), 'indices': [1, 0]}
  os.makedirs(str(tmp_path / '30'))
  c = analysis.CountAnalyzer(str(tmp_path / '30' / 'count.csv'))
  c.stage(res)
  assert open(c.fname).read() == ro.count_text([1, 0], y, s_gt)
  # the ground truth, coloured by its best match: the analyzer computes iou_pairwise when the dict has none
  g = analysis.RenderGroundtruthInstanceAnalyzer(str(tmp_path / 'gt'), names)
  with pytest.raises(IndexError):  # 23 outputs: the last one can win, and index 22 is beyond the palette, as in the reference
    g.stage(dict(res, iou_pairwise=np.eye(23, 4)[None].repeat(B, 0)[:, ::-1].copy()))
  assert 'iou_pairwise' not in res
  g.stage(res)
  iou = res['iou_pairwise'].cpu().numpy()
  assert iou.shape == (B, T, 4) and iou.any()
  want = ro.render_groundtruth(y_gt, iou)
  assert want.any()
  for b, f in enumerate(files('gt')):
    assert (png.read_colour8(f) == want[b]).all()
  # the orientation image from d_out at network size
  for k, shape in enumerate(ORI_SHAPES):
    d, mask, full, want, sure = _ori_case(shape)
    o = analysis.RenderOrientationAnalyzer(str(tmp_path / ('ori%d' % k)), names)
    o.stage({'d_out': _dev(d), 'mask': _dev(mask), 'indices': [0, 1]})
    for b, n in enumerate(('a_000_x', 'b_111_y')):
      got = png.read_colour8(str(tmp_path / ('ori%d' % k) / (n + '.png')))
      assert got.shape == want[b].shape and (got[sure[b]] == want[b][sure[b]]).all()


def test_full_model_eval_render(cuda, tmp_path):
  """full_model_eval.py --render --render_gt_instances on the configuration of test_eval_gpu's driver test (64 x 64, T = 4, three
  images with y_gt / s_gt): the per-threshold folders, gt/ and count.csv exist and the images are the oracle's for the chain's
  own y_bin."""
  import yaml
  import full_model
  import full_model_eval
  import full_model_train
  from test_loss_gpu import synth_gt
  from utils import postprocess as pp
  res = str(tmp_path / 'results')
  full_model_train.main(['--init_only', '--results', res, '--model_id', 'm0', '--inp_height', '64',
                         '--inp_width', '64', '--timespan', '4', '--ctrl_add_inp', '--ctrl_add_canvas',
                         '--attn_add_inp', '--attn_add_canvas', '--fixed_gamma',
                         '--ctrl_cnn_filter_size', '3,3,3,3', '--ctrl_cnn_depth', '8,8,16,16',
                         '--ctrl_cnn_pool', '1,2,1,2', '--attn_cnn_filter_size', '3,3,3,3,3,3',
                         '--attn_cnn_depth', '8,8,16,16,32,32', '--attn_cnn_pool', '1,2,1,2,1,2',
                         '--attn_dcnn_filter_size', '3,3,3,3,3,3,3', '--attn_dcnn_depth', '32,32,16,16,8,8,1',
                         '--attn_dcnn_pool', '2,1,2,1,2,1,1'])
  rng = np.random.RandomState(4)
  x = rng.rand(3, 64, 64, 3).astype(np.float32)
  y_gt, s_gt = synth_gt(rng, 3, 4, 64, 64, max_inst=3)
  inp = str(tmp_path / 'in.npz')
  np.savez(inp, x=x, y_gt=y_gt, s_gt=s_gt, names=np.array(['img_a.png', 'img_b.png', 'img_c.png']))
  thresholds = [0.3, 0.55]
  full_model_eval.main(['--model_id', 'm0', '--results', res, '--input', inp, '--batch_size', '2', '--threshold_list', '0.3,0.55',
                        '--analyzers', 'sbd', '--render', '--render_gt_instances'])
  out_dir = tmp_path / 'results' / 'm0' / 'output_valid'
  assert sorted(p.name for p in out_dir.iterdir() if p.is_dir()) == ['30', '55', 'gt']
  with open(str(tmp_path / 'results' / 'm0' / 'model_opt.yaml')) as f:
    opt = yaml.safe_load(f)
  opt['use_knob'] = False
  m = full_model.get_model(opt).load_weights(dict(np.load(str(tmp_path / 'results' / 'm0' / 'weights.npz'))))
  gt, sg = _dev(y_gt), _dev(s_gt)
  names = ['img_a', 'img_b', 'img_c']
  rows = {th: [] for th in thresholds}
  y_all, s_all = m.run(['y_out', 's_out'], {'x': x, 'phase_train': False})
  for b0, b1 in ((0, 2), (2, 3)):  # the driver's batches
    yc, s_hard = pp.apply_confidence(y_all[b0:b1].contiguous(), s_all[b0:b1].contiguous())
    one = pp.apply_one_label(pp.upsample(yc, gt[b0:b1]))
    for th in thresholds:
      y_bin = pp.apply_threshold(one, th)
      yb = y_bin.cpu().numpy()
      want = ro.render_instances(yb)
      for i in range(b0, b1):
        got = png.read_colour8(str(out_dir / ('%02d' % int(th * 100)) / (names[i] + '.png')))
        assert (got == want[i - b0]).all(), (th, i)
      rows[th].append(ro.count_text(list(range(b0, b1)), yb, s_gt[b0:b1]).split('\n', 1)[1])
    iou = analysis.f_iou_pairwise(y_bin, gt[b0:b1]).cpu().numpy()  # the last threshold's, as full_model_eval.py:139-140
    want = ro.render_groundtruth(y_gt[b0:b1], iou)
    for i in range(b0, b1):
      assert (png.read_colour8(str(out_dir / 'gt' / (names[i] + '.png'))) == want[i - b0]).all(), i
  for th in thresholds:
    text = open(str(out_dir / ('%02d' % int(th * 100)) / 'count.csv')).read()
    assert text == 'Image ID,Count Out,Count GT\n' + ''.join(rows[th])
  assert any(png.read_colour8(str(out_dir / 'gt' / (n + '.png'))).any() for n in names)


def test_cityscapes_eval_render_instances(cuda, tmp_path):
  """cityscapes_eval.py --render_instances: per threshold the instance image of iter_label_instances' y_out and count.csv, and
  gt/ from y_gt_full with the last threshold's pairwise IoU."""
  import cityscapes_eval as ce
  scenes = [cso.synthetic_scene(sd) for sd in (11, 12)]
  names = ['aachen_000001_000019.png', 'bochum_000001_000019']
  y, s, sem = (np.concatenate([sc[k] for sc in scenes]) for k in range(3))
  H, W = 128, 256
  gt = (cso.resize_linear(y, H, W) > 0.5).astype(np.float32)
  s_gt = np.ones(s.shape, np.float32)
  src, out = str(tmp_path / 'in.npz'), str(tmp_path / 'out')
  np.savez(src, y_out_ins=y, s_out=s, y_out=sem, y_gt_full=gt, s_gt=s_gt, names=np.array(names))
  ce.main(['--input', src, '--output', out, '--threshold_list', '0.3,0.5', '--remove_tiny', '120', '--analyzers', 'sbd',
           '--render_instances'])
  root = os.path.join(out, 'output_valid')
  chain = ce.label_instances(_dev(y), _dev(s), _dev(sem), (H, W), [0.3, 0.5], 120)
  for th, res in zip((30, 50), chain):
    y_bin = res['y_out'].cpu().numpy()
    want = ro.render_instances(y_bin)
    assert want.any()
    for i, n in enumerate(('aachen_000001_000019', 'bochum_000001_000019')):
      assert (png.read_colour8(os.path.join(root, '%02d' % th, n + '.png')) == want[i]).all()
    assert open(os.path.join(root, '%02d' % th, 'count.csv')).read() == ro.count_text([0, 1], y_bin, s_gt)
  iou = analysis.f_iou_pairwise(chain[-1]['y_out'], _dev(gt)).cpu().numpy()
  want = ro.render_groundtruth(gt, iou)
  for i, n in enumerate(('aachen_000001_000019', 'bochum_000001_000019')):
    assert (png.read_colour8(os.path.join(root, 'gt', n + '.png')) == want[i]).all()
  # without the flag nothing of it is written
  out2 = str(tmp_path / 'out2')
  ce.main(['--input', src, '--output', out2, '--threshold_list', '0.3', '--analyzers', ''])
  assert sorted(os.listdir(os.path.join(out2, 'output_valid'))) == ['cityscapes', 'metrics.yaml']


def test_fg_model_eval_render_orientation(cuda, tmp_path):
  """fg_model_eval.py --render_orientation: <output>/ori/<name>.png from the model's d_out and fg_gt_full > 0; a model without
  add_orientation is refused by name."""
  import yaml
  import fg_eval_oracle as feo
  import fg_model_eval
  import fg_model_pack
  import fg_oracle as fo
  res = str(tmp_path / 'results')
  for mid, ori in (('fg', True), ('plain', False)):
    opt = dict(fo.reduced_opt(1, ori), segm_loss_fn='bce')
    os.makedirs(os.path.join(res, mid))
    with open(os.path.join(res, mid, 'model_opt.yaml'), 'w') as f:
      yaml.safe_dump(opt, f)
    np.savez(os.path.join(res, mid, 'weights.npz'), step=np.float32(1), **fo.random_weights(opt, 61))
  rng = np.random.RandomState(62)
  N, h, w, H, W = 3, 32, 48, 61, 103
  x = rng.rand(N, h, w, 3).astype(np.float32)
  gt = feo.disc_labels(rng, N, H, W)
  src, out = str(tmp_path / 'in.npz'), str(tmp_path / 'out')
  np.savez(src, x=x, fg_gt_full=gt, names=np.array(['a.png', 'b.png', 'c.png']))
  fg_model_eval.main(['--model_id', 'fg', '--results', res, '--input', src, '--output', out, '--batch_size', '2',
                      '--render_orientation'])
  d = fg_model_pack.restore_model(res, 'fg').run('d_out', {'x': x, 'phase_train': False}).cpu().numpy()
  full = ro.orientation_full(d, H, W)
  mask = (gt > 0).astype(np.float32)
  want, sure = ro.orientation_image(full, mask), ro.orientation_gap(full) >= GAP
  assert want.any() and (mask == 0).any()
  for i, n in enumerate('abc'):
    got = png.read_colour8(os.path.join(out, 'ori', n + '.png'))
    assert got.shape == (H, W, 3) and (got[sure[i]] == want[i][sure[i]]).all()
  assert not os.path.exists(os.path.join(out, '30', 'ori'))
  with pytest.raises(rn.RecAttendError, match='add_orientation'):
    fg_model_eval.main(['--model_id', 'plain', '--results', res, '--input', src, '--output', out, '--render_orientation'])
