"""The Cityscapes output stage on the MI355X: the foreground mask of the semantic map (ra_sem_foreground_f32), the class vote
(ra_instance_class_vote_f32) and the pick against the float64 oracle of tests/cs_oracle.py, label_instances end to end on a
synthetic scene, and the two command lines.  Bars: 2e-5 relative to the largest reference value for the vote (the project's
kernel bar: every term is a product of values in [0, 1], so nothing cancels, and the resize holds 2e-6 absolute); decisions
(foreground, pick, masks) are compared wherever the oracle's value is not within the resize bar of the decision's threshold,
and how many values that leaves out is itself asserted on the oracle alone."""
import functools
import os

import numpy as np
import pytest
import torch

import cs_oracle as co
import ra_native as rn
import ra_ops as ops
import ra_oracle as ora

pytestmark = pytest.mark.gpu
TOL = 2e-5        # tests/test_fg_model_gpu.py TOL
RESIZE_BAR = 2e-6  # tests/test_eval_gpu.py: the upsample's absolute bar


def _dev(a):
  return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


# id -> (B, T, (Hs, Ws), (H, W), C, soft)
VOTE_CASES = {
    'cityscapes': (1, 20, (256, 512), (1024, 2048), 9, False),
    'small_soft': (3, 8, (48, 80), (96, 160), 9, True),
    'small_binary': (3, 8, (48, 80), (96, 160), 9, False),
    'ratio': (2, 5, (48, 80), (100, 180), 9, True),       # a non-integer ratio
    'c2': (2, 4, (24, 40), (96, 160), 2, True),
    'c16_t32': (2, 32, (24, 40), (48, 80), 16, True),
    'w_odd': (2, 3, (25, 45), (50, 90), 9, True),         # W % 4 != 0, H * W % 4 == 0: 16-byte loads that cross row ends
    'hw_odd': (1, 3, (20, 20), (45, 45), 9, False),       # H * W % 4 != 0: element loads
    't1': (1, 1, (16, 16), (40, 24), 9, True),
}


@functools.lru_cache(maxsize=None)
def _vote_case(name):
  B, T, (Hs, Ws), (H, W), C, soft = VOTE_CASES[name]
  rng = np.random.RandomState(sorted(VOTE_CASES).index(name) + 50)
  sem = co.smooth_semantic_map(rng, B, Hs, Ws, C)
  y = co.disc_instances(rng, B, T, H, W, soft=soft)
  conf = rng.uniform(0.3, 1.0, (B, T)).astype(np.float32)
  ref = co.vote(y, co.sem_full(sem, H, W))
  return y, sem, conf, ref


@pytest.mark.parametrize('name', sorted(VOTE_CASES))
def test_vote_matches_float64_oracle(cuda, name):
  y, sem, conf, ref = _vote_case(name)
  assert ref.max() > 1e-3 and (ref[..., 1:].max(axis=-1) > 0).mean() > 0.5  # empty instances would pass any tolerance
  got = ops.instance_class_vote(_dev(y), _dev(sem)).cpu().numpy()
  assert got.shape == ref.shape and got.dtype == np.float32
  err = np.abs(got - ref).max() / np.abs(ref).max()
  print('vote %s %s: max|got - ref| / max|ref| = %.3g (max|ref| = %.4f)' % (name, VOTE_CASES[name], err, ref.max()))
  assert err <= TOL, (name, err)


@pytest.mark.parametrize('name', ['cityscapes', 'small_soft', 'hw_odd'])
def test_vote_is_run_to_run_identical(cuda, name):
  y, sem, conf, _ = _vote_case(name)
  y, sem, conf = _dev(y), _dev(sem), _dev(conf)
  a = ops.instance_class_vote(y, sem, conf)
  b = ops.instance_class_vote(y, sem, conf)
  assert all(torch.equal(u, v) for u, v in zip(a, b))
  assert torch.equal(a[0], ops.instance_class_vote(y, sem))  # the vote does not depend on the pick riding along


def _check_pick(name, ref_vote, conf, got_idx, got_lab, exclude=True):
  """class_idx / label_id equal the oracle's for every instance whose two largest class votes differ by more than 1e-4 * the
  largest vote in the oracle (five times the vote bar); at most one scored instance may be left out."""
  ref_idx, ref_lab = co.pick(ref_vote, conf)
  clear = co.top2_gap(ref_vote) > 1e-4 * ref_vote.max() if exclude else np.ones(conf.shape, bool)
  left = (conf > 0.5) & ~clear
  print('pick %s: %d of %d scored instances within 1e-4 * max vote of a tie' % (name, left.sum(), (conf > 0.5).sum()))
  assert left.sum() <= 1
  assert (conf > 0.5).sum() >= 1
  assert np.array_equal(got_idx[~left], ref_idx[~left]), (name, got_idx, ref_idx)
  assert np.array_equal(got_lab[~left], ref_lab[~left]), (name, got_lab, ref_lab)
  assert set(np.unique(got_lab)) <= {-1} | {l for _, l in co.LABELS}


@pytest.mark.parametrize('name', sorted(VOTE_CASES))
def test_pick_matches_oracle(cuda, name):
  y, sem, conf, ref = _vote_case(name)
  vote, idx, lab = ops.instance_class_vote(_dev(y), _dev(sem), _dev(conf))
  assert idx.dtype == torch.int32 and lab.dtype == torch.int32
  _check_pick(name, ref, conf, idx.cpu().numpy(), lab.cpu().numpy())
  idx2, lab2 = ops.instance_class_pick(vote, _dev(conf))  # the stand-alone launch = the tail of the finishing launch
  assert torch.equal(idx2, idx) and torch.equal(lab2, lab)


def test_pick_exact_tie_and_empty_instance(cuda):
  rng = np.random.RandomState(77)
  B, T, Hs, Ws, H, W, C = 2, 6, 24, 40, 96, 160, 5
  a = co.smooth_semantic_map(rng, B, Hs, Ws, 3)
  sem = np.zeros((B, Hs, Ws, C), np.float32)
  sem[..., 0] = 0.1
  sem[..., 1] = 0.05
  sem[..., 2] = 0.3 + 0.5 * a[..., 1]   # channels 2 and 4 are identical: an exact tie, the first wins (class index 1)
  sem[..., 4] = sem[..., 2]
  sem[..., 3] = 0.1 * a[..., 2]
  y = co.disc_instances(rng, B, T, H, W, soft=True)
  y[:, 3] = 0.0                          # an all-zero instance with a score: written as the first class, like numpy.argmax
  conf = np.full((B, T), 0.9, np.float32)
  conf[:, 5] = 0.5                       # exactly 0.5 is not written
  ref = co.vote(y, co.sem_full(sem, H, W))
  assert (ref[..., 2] == ref[..., 4]).all() and (ref[:, :3, 2] > ref[:, :3, 3]).all() and (ref[:, 3] == 0).all()
  vote, idx, lab = ops.instance_class_vote(_dev(y), _dev(sem), _dev(conf))
  v = vote.cpu().numpy()
  assert (v[..., 2] == v[..., 4]).all() and (v[:, 3] == 0).all()
  ref_idx, ref_lab = co.pick(ref, conf)
  assert ref_idx[:, :3].tolist() == [[1] * 3] * B and ref_idx[:, 3].tolist() == [0] * B and ref_idx[:, 5].tolist() == [-1] * B
  assert np.array_equal(idx.cpu().numpy(), ref_idx) and np.array_equal(lab.cpu().numpy(), ref_lab)  # no exclusion here
  idx2, lab2 = ops.instance_class_pick(vote, _dev(conf))
  assert torch.equal(idx2, idx) and torch.equal(lab2, lab)


def test_other_shapes_are_refused(cuda):
  sem = torch.zeros(1, 8, 8, 9, device='cuda')
  with pytest.raises(rn.RecAttendError, match='T=33'):
    ops.instance_class_vote(torch.zeros(1, 33, 16, 16, device='cuda'), sem)
  with pytest.raises(rn.RecAttendError, match='C=17'):
    ops.instance_class_vote(torch.zeros(1, 2, 16, 16, device='cuda'), torch.zeros(1, 8, 8, 17, device='cuda'))
  with pytest.raises(rn.RecAttendError, match='C=1'):
    ops.instance_class_vote(torch.zeros(1, 2, 16, 16, device='cuda'), torch.zeros(1, 8, 8, 1, device='cuda'))
  with pytest.raises(rn.RecAttendError):
    ops.instance_class_vote(torch.zeros(2, 2, 16, 16, device='cuda'), sem)  # batch sizes differ


# ---- the foreground mask
@pytest.mark.parametrize('seed', [0, 1])
@pytest.mark.parametrize('shape', [((256, 512), (1024, 2048)), ((48, 80), (96, 160)), ((48, 80), (100, 180))],
                         ids=['cityscapes', 'x2', 'ratio'])
@pytest.mark.parametrize('C', [9, 1])
def test_sem_foreground(cuda, shape, seed, C):
  (Hs, Ws), (H, W) = shape
  sem = co.smooth_semantic_map(np.random.RandomState(seed), 2, Hs, Ws, 9)
  if C == 1:  # a one-channel foreground map: 1 - background, through the same 8-bit round trip; the rule is > 0.3 then
    sem = (np.float32(1) - sem[..., :1])
    sem = ((sem * 255).astype('uint8').astype('float32') / np.float32(255))
  sem_h = co.sem_full(sem, H, W)
  ref = co.foreground(sem_h)
  lim = co.FG_THRESHOLD if C == 1 else 1 - co.FG_THRESHOLD
  clear = np.abs(sem_h[..., 0] - lim) > RESIZE_BAR
  print('sem_foreground %s C=%d seed %d: %.4f %% of the pixels within 2e-6 of the threshold; foreground %.1f %%' % (
      shape, C, seed, 100 * (1 - clear.mean()), 100 * ref.mean()))
  assert 1 - clear.mean() <= 1e-3
  assert 0.1 <= ref.mean() <= 0.9  # a map that never crosses the threshold tests nothing
  got = ops.sem_foreground(_dev(sem), H, W, co.FG_THRESHOLD).cpu().numpy()
  assert got.shape == ref.shape and set(np.unique(got)) <= {0.0, 1.0}
  assert np.array_equal(got[clear], ref[clear].astype(np.float32))


# ---- label_instances end to end
SCENE_SEED, SCENE_TINY = 11, 120
THRESHOLDS = [i * 0.1 for i in range(10)]


def test_label_instances_end_to_end(cuda):
  import cityscapes_eval as ce
  y, s, sem, classes = co.synthetic_scene(SCENE_SEED)
  H, W = 128, 256
  assert s[0, 1] == np.float32(0.2) and s[0, 2] == 0.5 and (y == 0).mean() > 0.5
  ref = co.label_instances(y, s, sem, (H, W), THRESHOLDS, SCENE_TINY)
  got = ce.label_instances(_dev(y), _dev(s), _dev(sem), (H, W), THRESHOLDS, SCENE_TINY)
  assert len(got) == len(THRESHOLDS)
  v = ref['one'].max(axis=1)                                   # the one-label value of every pixel
  srt = np.sort(ref['y_conf'], axis=1)
  near_tie = (srt[:, -1] - srt[:, -2] < 2 * RESIZE_BAR) & (srt[:, -1] > 0)  # where every instance is exactly 0 nothing is decided
  fg_clear = np.abs(ref['sem_h'][..., 0] - (1 - co.FG_THRESHOLD)) > RESIZE_BAR
  assert fg_clear.all()  # the scene's background levels cannot land on 0.7: the foreground mask is decided everywhere
  assert np.array_equal(got[0]['fg'].cpu().numpy(), ref['fg'].astype(np.float32)) and 0.1 < ref['fg'].mean() < 0.9
  removed_somewhere = False
  for g, r in zip(got, ref['per_threshold']):
    th = r['threshold']
    assert g['threshold'] == th
    d = np.abs(v - th)
    left = ((d > 0) & (d <= RESIZE_BAR)) | near_tie   # [1,H,W]
    n_left = int(left.sum())
    print('label_instances th %.1f: %d pixels (%.3f %%) left out; sizes %s' % (th, n_left, 100 * left.mean(),
                                                                              r['sizes'][0].astype(int).tolist()))
    assert left.mean() <= 5e-3
    assert (np.abs(r['sizes'] - SCENE_TINY) > n_left).all()       # remove_tiny decides the same on both sides
    keep = np.broadcast_to(~left[:, None], r['y_out'].shape)
    gy = g['y_out'].cpu().numpy()
    assert np.array_equal(gy[keep], r['y_out'][keep].astype(np.float32)), th
    assert np.array_equal(g['conf'].cpu().numpy(), r['conf'].astype(np.float32)), th
    assert np.array_equal(g['s_out'].cpu().numpy(), ref['conf_hard'].astype(np.float32))
    _check_pick('scene th %.1f' % th, r['vote'], r['conf'], g['class_idx'].cpu().numpy(), g['label_id'].cpu().numpy())
    err = np.abs(g['vote'].cpu().numpy() - r['vote']).max()
    assert err <= TOL * r['vote'].max() + n_left / float(H * W)  # a left-out pixel moves a vote by at most 1 / HW
    written = r['class_idx'][0] >= 0
    written[-1] = False  # the tiny last disc lies inside its neighbour's class region
    assert np.array_equal(r['class_idx'][0][written], classes[written])  # the oracle finds the classes the scene was built with
    removed_somewhere |= bool(((r['conf'] == 0) & (r['sizes'] > SCENE_TINY)).any())
  assert (ref['per_threshold'][0]['class_idx'] >= 0).sum() >= 4
  # conf is carried from threshold to threshold: with a list that comes back DOWN, an instance that was tiny at 0.6 is large
  # enough again at 0.0 and still has conf = 0 there (an implementation that started every threshold from s_out would write it)
  ref2 = co.label_instances(y, s, sem, (H, W), [0.6, 0.0], SCENE_TINY)['per_threshold']
  got2 = ce.label_instances(_dev(y), _dev(s), _dev(sem), (H, W), [0.6, 0.0], SCENE_TINY)
  back = (ref2[1]['conf'] == 0) & (ref2[1]['sizes'] > SCENE_TINY) & (s > 0.5)
  assert back.any() and (np.abs(ref2[1]['sizes'] - SCENE_TINY) > 12).all() and (np.abs(ref2[0]['sizes'] - SCENE_TINY) > 12).all()
  for g, r in zip(got2, ref2):
    assert np.array_equal(g['conf'].cpu().numpy(), r['conf'].astype(np.float32))
    assert np.array_equal(g['class_idx'].cpu().numpy()[back], r['class_idx'][back]) and (r['class_idx'][back] == -1).all()


# ---- the command lines
def _parse_txt(path):
  out = []
  for line in open(path).read().splitlines():
    f, lab, score = line.split(' ')
    out.append((f, int(lab), score))
  return out


def test_cityscapes_eval_command_line(cuda, tmp_path):
  import yaml
  import cityscapes_eval as ce
  from utils import png
  scenes = [co.synthetic_scene(sd) for sd in (11, 12, 13)]
  names = ['aachen_000001_000019.png', 'aachen_000002_000019.png', 'bochum_000001_000019']
  y = np.concatenate([sc[0] for sc in scenes])
  s = np.concatenate([sc[1] for sc in scenes])
  sem = np.concatenate([sc[2] for sc in scenes])
  H, W = 128, 256
  gt = (co.resize_linear(y, H, W) > 0.5).astype(np.float32)
  src, out = str(tmp_path / 'in.npz'), str(tmp_path / 'out')
  np.savez(src, y_out_ins=y, s_out=s, y_out=sem, y_gt_full=gt, s_gt=np.ones(s.shape, np.float32), names=np.array(names))
  ths = [0.3, 0.5]
  renders = ce.main(['--input', src, '--output', out, '--threshold_list', '0.3,0.5', '--remove_tiny', '120', '--batch_size', '2',
                     '--analyzers', 'sbd,wt_cov,fg_iou,dic'])
  assert len(renders) == 2
  root = os.path.join(out, 'output_valid', 'cityscapes')
  metrics = yaml.safe_load(open(os.path.join(out, 'output_valid', 'metrics.yaml')))
  assert sorted(metrics) == ['0.30', '0.50'] and metrics['0.30']['sbd']['count'] == 3 and 0 < metrics['0.30']['sbd']['mean'] <= 1
  final = ce.label_instances(_dev(y), _dev(s), _dev(sem), (H, W), ths, 120)[-1]   # what remains on disk: the last threshold
  idx, lab = final['class_idx'].cpu().numpy(), final['label_id'].cpu().numpy()
  conf, masks = final['conf'].cpu().numpy(), final['y_out'].cpu().numpy()
  n_written = 0
  for i, name in enumerate(names):
    stem = name[:-4] if name.endswith('.png') else name
    folder = os.path.join(root, stem.split('_')[0])
    lines = _parse_txt(os.path.join(folder, stem + '.txt'))
    want = [('%s_%03d.png' % (stem, t), int(lab[i, t]), '%f' % conf[i, t]) for t in range(idx.shape[1]) if idx[i, t] >= 0]
    assert lines == want
    for f, label, _ in lines:
      assert label in [l for _, l in co.LABELS]
      t = int(f[-7:-4])
      img = png.read_gray8(os.path.join(folder, f))
      assert img.dtype == np.uint8 and np.array_equal(img, (masks[i, t] * 255).astype('uint8')) and img.max() == 255
      n_written += 1
  assert n_written >= 6
  # the images of a split (:41-46)
  out2 = str(tmp_path / 'out2')
  ce.main(['--input', src, '--output', out2, '--threshold_list', '0.3', '--split_id', '1', '--num_split', '2', '--analyzers', ''])
  found = sorted(os.listdir(os.path.join(out2, 'output_valid', 'cityscapes')))
  assert found == ['bochum']


def _small_fg_opt9():
  return dict(inp_depth=3, cnn_filter_size=[3] * 4, cnn_depth=[8, 16, 144, 32], cnn_pool=[1, 2, 2, 1],
              cnn_skip_mask=[True, False, True, False], dcnn_filter_size=[3] * 4, dcnn_depth=[160, 16, 8, 17], dcnn_pool=[2, 1, 2, 1],
              dcnn_skip_mask=[False, True, True], use_bn=True, add_skip_conn=True, add_orientation=True, num_orientation_classes=8,
              num_semantic_classes=9, weight_decay=5e-5)


def test_full_model_eval_cityscapes_output(cuda, tmp_path):
  """The score head's bias is raised so that the random decode net scores its instances above 0.5, and the images are made of
  coloured blocks so that the random pre-stage votes for different classes in different images: the float64 oracles of the two
  nets put ten instances of the classes person, rider and bus into the five text files at the last threshold, with the two
  largest votes of the rider / bus / person instances of images 0, 1 and 3 at least 2 % of the largest vote apart."""
  import yaml
  import cityscapes_eval as ce
  import fg_model_pack
  import fg_oracle as fo
  import full_model
  import full_model_eval
  res = str(tmp_path / 'results')
  fopt = _small_fg_opt9()
  os.makedirs(os.path.join(res, 'fg'))
  with open(os.path.join(res, 'fg', 'model_opt.yaml'), 'w') as f:
    yaml.safe_dump(fopt, f)
  np.savez(os.path.join(res, 'fg', 'weights.npz'), step=np.float32(1), **fo.random_weights(fopt, 31))
  opt = ora.make_opt('cityscapes', 64, 96, 3)
  os.makedirs(os.path.join(res, 'full'))
  with open(os.path.join(res, 'full', 'model_opt.yaml'), 'w') as f:
    yaml.safe_dump({k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in opt.items()}, f)
  P = ora.random_params(opt, 4)
  P['score_mlp_b_0'] = P['score_mlp_b_0'] + 3.0
  np.savez(os.path.join(res, 'full', 'weights.npz'), **full_model.get_model(opt).load_weights(P).state_dict_numpy())
  src, packed = str(tmp_path / 'in.npz'), str(tmp_path / 'packed.npz')
  rng = np.random.RandomState(9)
  x = np.kron(rng.rand(5, 2, 3, 3).transpose(0, 3, 1, 2), np.ones((32, 32))).transpose(0, 2, 3, 1) * 0.8 + 0.2 * rng.rand(5, 64, 96, 3)
  np.savez(src, x=x.astype(np.float32))
  a, b, d = str(tmp_path / 'a'), str(tmp_path / 'b'), str(tmp_path / 'cs')
  common = ['--model_id', 'full', '--results', res, '--input', src, '--batch_size', '2', '--test', '--fg_model_id', 'fg',
            '--threshold_list', '0.0,0.3', '--remove_tiny', '20']
  full_model_eval.main(common + ['--output', a, '--cityscapes_output', d])
  full_model_eval.main(common + ['--output', b])
  pa = os.path.join(a, os.listdir(a)[0], 'pred_rank0.npz')
  pb = os.path.join(b, os.listdir(b)[0], 'pred_rank0.npz')
  ra, rb = np.load(pa), np.load(pb)
  assert sorted(ra.files) == sorted(rb.files) == ['first_index', 's_out', 'y_out']
  assert ra['y_out'].shape == (5, 3, 64, 96)
  assert all(np.array_equal(ra[k], rb[k]) and ra[k].dtype == rb[k].dtype for k in ra.files)  # the flag leaves the outputs alone
  # the same classes as the stand-alone stage fed with that run's outputs and the pack step's y_in
  fg_model_pack.main(['--model_id', 'fg', '--results', res, '--input', src, '--output', packed, '--batch_size', '2'])
  y_in = np.load(packed)['y_in']
  assert y_in.shape == (5, 64, 96, 9)
  stage_in, c = str(tmp_path / 'stage.npz'), str(tmp_path / 'c')
  np.savez(stage_in, y_out_ins=ra['y_out'], s_out=ra['s_out'], y_out=y_in)
  ce.main(['--input', stage_in, '--output', c, '--threshold_list', '0.0,0.3', '--remove_tiny', '20', '--batch_size', '2'])
  n_lines, labels = 0, set()
  for i in range(5):
    ta = open(os.path.join(d, 'image', 'image_%06d.txt' % i)).read()
    tc = open(os.path.join(c, 'output_valid', 'cityscapes', 'image', 'image_%06d.txt' % i)).read()
    assert ta == tc, i
    n_lines += len(ta.splitlines())
    labels |= {int(line.split(' ')[1]) for line in ta.splitlines()}
    for line in ta.splitlines():  # and the masks are the same files
      f = line.split(' ')[0]
      assert open(os.path.join(d, 'image', f), 'rb').read() == open(os.path.join(c, 'output_valid', 'cityscapes', 'image', f), 'rb').read()
  print('full_model_eval --cityscapes_output: %d instances written for 5 images, label ids %s' % (n_lines, sorted(labels)))
  assert (ra['s_out'] > 0.5).sum() >= 10 and n_lines >= 6 and len(labels) >= 2
  assert labels <= {l for _, l in co.LABELS}
  # a pre-stage without the 9 classes is refused
  fopt1 = dict(fopt, num_semantic_classes=1, dcnn_depth=[160, 16, 8, 9])
  os.makedirs(os.path.join(res, 'fg1'))
  with open(os.path.join(res, 'fg1', 'model_opt.yaml'), 'w') as f:
    yaml.safe_dump(fopt1, f)
  np.savez(os.path.join(res, 'fg1', 'weights.npz'), step=np.float32(1), **fo.random_weights(fopt1, 31))
  with pytest.raises(rn.RecAttendError, match='9 semantic classes'):
    full_model_eval.main(['--model_id', 'full', '--results', res, '--input', src, '--fg_model_id', 'fg1', '--cityscapes_output', d])
