"""The Cityscapes output stage behind a label-image segmentation on the device (csrc/ra_label_vote.hip): the sweep's integer
counts and everything its finishing launch derives against the NumPy oracle (tests/label_vote_oracle.py) — exactly — the
planes against the existing ops' composition, the whole iterator against the existing one fed the one-hot map, the refusals,
and the command line end to end."""
import json
import os

import numpy as np
import pytest
import torch

import label_vote_oracle as lo
import ra_native as rn

pytestmark = pytest.mark.gpu

DEFAULT_LIST = [i * 0.1 for i in range(10)]                    # cityscapes_eval.py's default --threshold_list
SIXTEEN = [0.1, 0.7, 0.45, -0.1, 0.9, 0.3, 0.0, 0.7, 0.55, 0.2, 0.8, 0.35, 0.6, 0.05, 0.95, 0.5]  # unsorted, 0.7 twice, one negative
LISTS = {1: [0.3], 3: [0.5, -0.1, 0.5], 10: DEFAULT_LIST, 16: SIXTEEN}
#        B  T   H   W   K   remove_tiny (chosen on the host so that it drops some planes and keeps some; case 0 has one plane)
CASES = [(1, 1, 5, 7, 1, 1),        # H * W % 4 != 0: element loads, a tail
         (2, 3, 5, 7, 3, 4),
         (1, 20, 16, 64, 10, 20),   # one vector tile, the default list
         (3, 32, 33, 64, 16, 30)]   # both maxima, a partial last tile, several workgroups per image
CASE_ID = lambda c: 'B%d_T%d_%dx%d_K%d' % c[:5]


def _dev(a):
  return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(d):
  return {k: v.cpu().numpy() for k, v in d.items()}


def _scene(case):
  B, T, H, W, K, _ = case
  y, labels, conf = lo.scene(100 + T + K, B, T, H, W, LISTS[K])
  return y, labels, conf, LISTS[K]


def _check_inputs(y, labels, lut, ths):
  """The scene holds what the sweep must get right (asserted on the host, so the cases cannot vanish)."""
  am, v = lo.one_label(y)
  cls = lut[labels]
  assert (labels == 255).any() and ((cls == 0) & (labels != 255)).any() and (cls > 0).any()
  if y.shape[1] > 1:
    tied = (y == v[:, None]).sum(axis=1) > 1
    assert tied.any() and ((y == 0).all(axis=1) & (cls > 0)).any() and (am[(y == 0).all(axis=1)] == 0).all()
  for th in ths:
    f = np.float32(th)
    assert (v == f).any() and (v == np.nextafter(f, np.float32(np.inf), dtype=np.float32)).any(), th


def _compare(got, ref):
  assert got['counts'].dtype == np.int32 and np.array_equal(got['counts'], ref['counts'])
  for k in ('sizes', 'keep', 'class_idx', 'label_id'):
    assert np.array_equal(got[k], ref[k]), k
  assert np.array_equal(got['conf'], ref['conf']) and got['conf'].dtype == np.float32
  assert (np.abs(got['vote'].astype(np.float64) - ref['vote']) <= np.spacing(ref['vote'])).all()   # 1 ulp of float32
  assert (got['vote'][..., 0] == 0).all()


@pytest.mark.parametrize('case', CASES, ids=CASE_ID)
def test_sweep_equals_the_oracle(cuda, case):
  import ra_ops as ops
  y, labels, conf, ths = _scene(case)
  lut = ops.label_class_lut('labelIds')
  _check_inputs(y, labels, lut, ths)
  yd, ld, cd = _dev(y), _dev(labels), _dev(conf)
  for remove_tiny in (0, case[5]):
    ref = lo.sweep(y, labels, lut, ths, conf, remove_tiny)
    first = ops.label_vote_sweep(yd, ld, lut, ths, cd, remove_tiny)
    again = ops.label_vote_sweep(yd, ld, lut, ths, cd, remove_tiny)
    assert all(torch.equal(first[k], again[k]) for k in first)      # two runs, identical bits
    _compare(_host(first), ref)
    if remove_tiny:
      assert 0 < ref['keep'].sum() < ref['keep'].size or case[1] == 1   # the bound drops some planes, not all
  if len(ths) > 1 and min(ths) < 0:  # the negative threshold: every foreground pixel of an all-zero column goes to instance 0
    k = ths.index(min(ths))
    dead = (y == 0).all(axis=1) & (lut[labels] > 0)
    assert dead.any() and ref['counts'][k, :, 0].sum() >= dead.sum()


def test_sweep_on_an_unaligned_view(cuda):
  """y one float off a 16-byte boundary: the element-load path at a size the vector path would take."""
  import ra_ops as ops
  case = CASES[2]
  y, labels, conf, ths = _scene(case)
  lut = ops.label_class_lut('labelIds')
  buf = torch.zeros(y.size + 1, dtype=torch.float32, device='cuda')
  yd = buf[1:].view(y.shape)
  yd.copy_(_dev(y))
  assert yd.data_ptr() % 16 == 4 and yd.is_contiguous()
  lbuf = torch.zeros(labels.size + 1, dtype=torch.uint8, device='cuda')
  ld = lbuf[1:].view(labels.shape)
  ld.copy_(_dev(labels))
  _compare(_host(ops.label_vote_sweep(yd, ld, lut, ths, _dev(conf), 20)), lo.sweep(y, labels, lut, ths, conf, 20))
  keep = _dev((np.arange(case[1]) % 3 != 0).astype(np.uint8)[None])
  assert np.array_equal(ops.label_planes(yd, ld, lut, 0.3, keep=keep).cpu().numpy(), lo.planes(y, labels, lut, 0.3, keep.cpu().numpy()))


def test_count_above_2_pow_24(cuda):
  """Every pixel of a 4096 x 4100 image in one instance and one class: 16 793 600, which no float32 accumulator holds."""
  import ra_ops as ops
  H, W = 4096, 4100
  y = torch.ones(1, 1, H, W, device='cuda')
  labels = torch.full((1, H, W), 26, dtype=torch.uint8, device='cuda')
  out = _host(ops.label_vote_sweep(y, labels, ops.label_class_lut('labelIds'), [0.5], torch.ones(1, 1, device='cuda'), 400))
  assert H * W == 16793600 > 1 << 24 and int(np.float32(H * W - 1)) != H * W - 1
  assert out['counts'][0, 0, 0].tolist() == [0, 0, H * W, 0, 0, 0, 0, 0] and out['sizes'][0, 0, 0] == H * W
  assert out['vote'][0, 0, 0].tolist() == [0, 0, 0, 1.0, 0, 0, 0, 0, 0] and out['label_id'][0, 0, 0] == 26 and out['keep'].all()
  labels[0, -1, -1] = 7   # one pixel fewer: a count a float32 cannot represent
  out = _host(ops.label_vote_sweep(y, labels, ops.label_class_lut('labelIds'), [0.5], torch.ones(1, 1, device='cuda'), 400))
  assert out['counts'][0, 0, 0, 2] == H * W - 1 == out['sizes'][0, 0, 0]


@pytest.mark.parametrize('case', CASES, ids=CASE_ID)
def test_planes(cuda, case):
  """label_planes against the oracle at every shape and, where the existing ops run (H * W % 4 == 0), bit-equal to
  apply_one_label -> apply_threshold -> mask_foreground -> remove_tiny on the same y and the same fg."""
  import ra_ops as ops
  from utils import postprocess as pp
  y, labels, conf, ths = _scene(case)
  B, T, H, W, _, remove_tiny = case
  lut = ops.label_class_lut('labelIds')
  yd, ld, cd = _dev(y), _dev(labels), _dev(conf)
  for th in ths[:4]:
    keep = ops.label_vote_sweep(yd, ld, lut, [th], cd, remove_tiny)['keep'][0]
    for kp in (None, keep):
      got = ops.label_planes(yd, ld, lut, th, keep=kp)
      assert got.dtype == torch.float32 and got.shape == yd.shape
      assert np.array_equal(got.cpu().numpy(), lo.planes(y, labels, lut, th, None if kp is None else kp.cpu().numpy()))
      if (H * W) % 4 == 0 and th >= 0:
        fg = _dev((lut[labels] > 0).astype(np.float32))
        chain = pp.mask_foreground(pp.apply_threshold(pp.apply_one_label(yd), float(th)), fg)
        if kp is not None:
          chain, _ = pp.remove_tiny(chain, cd, threshold=remove_tiny)
        assert torch.equal(got.view(torch.int32), chain.view(torch.int32))   # the same bits


def test_iterator_equals_the_existing_one_on_the_one_hot_map(cuda):
  """A second, independent device reference: iter_label_instances fed the full-size one-hot map (the resize at equal size is
  the identity, and at 32 x 64 its float means are exact) gives the same label_id, conf and y_out per threshold."""
  import cityscapes_eval as ce
  ths = [0.0, 0.3, 0.5, 0.7, 0.3]
  y, labels, conf = lo.scene(7, 2, 6, 32, 64, ths)
  y = np.abs(y)
  lut = lo.class_lut('labelIds')
  sem = lo.onehot(labels, lut).astype(np.float32)
  old = list(ce.iter_label_instances(_dev(y), _dev(conf), _dev(sem), (32, 64), ths, remove_tiny=30))
  new = list(ce.iter_label_instances_from_labels(_dev(y), _dev(conf), _dev(labels), (32, 64), ths, remove_tiny=30))
  assert len(old) == len(new) == len(ths)
  n_written = 0
  for a, b in zip(old, new):
    assert set(a) <= set(b) and a['threshold'] == b['threshold'] and b['y_in'] is None and b['labels'].dtype == torch.uint8
    assert torch.equal(a['y_out'], b['y_out']) and torch.equal(a['conf'], b['conf']) and torch.equal(a['fg'], b['fg'])
    assert torch.equal(a['label_id'], b['label_id']) and torch.equal(a['class_idx'], b['class_idx']) and torch.equal(a['s_out'], b['s_out'])
    area = b['y_out'].sum(dim=(2, 3))
    assert ((area == b['sizes']) | ((area == 0) & (b['sizes'] <= 30))).all()   # sizes: before remove_tiny
    assert (a['vote'] - b['vote']).abs().max().item() <= 2.0 ** -24
    n_written += int((b['label_id'] >= 0).sum())
  assert n_written > 0 and (new[1]['conf'] == 0).any() and (new[1]['conf'] > 0).any()
  lean = list(ce.iter_label_instances_from_labels(_dev(y), _dev(conf), _dev(labels), (32, 64), ths, remove_tiny=30, planes=False))
  assert all(r['y_out'] is None and torch.equal(r['label_id'], b['label_id']) and torch.equal(r['conf'], b['conf'])
             for r, b in zip(lean, new))
  # more thresholds than one sweep takes: conf carries from one sweep into the next
  many = [0.05 * i for i in range(20)]
  a = list(ce.iter_label_instances(_dev(y), _dev(conf), _dev(sem), (32, 64), many, remove_tiny=30))
  b = list(ce.iter_label_instances_from_labels(_dev(y), _dev(conf), _dev(labels), (32, 64), many, remove_tiny=30, planes=False))
  assert len(b) == 20 and all(torch.equal(p['conf'], q['conf']) and torch.equal(p['label_id'], q['label_id']) for p, q in zip(a, b))


def test_refusals_name_the_argument(cuda):
  import ra_ops as ops
  lut = ops.label_class_lut('labelIds')
  z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device='cuda')
  y, labels, conf = z(1, 2, 4, 4), z(1, 4, 4, dt=torch.uint8), z(1, 2)
  with pytest.raises(rn.RecAttendError, match='label_vote_sweep: y has T = 33'):
    ops.label_vote_sweep(z(1, 33, 4, 4), labels, lut, [0.5], z(1, 33), 0)
  with pytest.raises(rn.RecAttendError, match='label_planes: y has T = 33'):
    ops.label_planes(z(1, 33, 4, 4), labels, lut, 0.5)
  with pytest.raises(rn.RecAttendError, match='thresholds has K = 17'):
    ops.label_vote_sweep(y, labels, lut, [0.01 * i for i in range(17)], conf, 0)
  with pytest.raises(rn.RecAttendError, match='thresholds has K = 0'):
    ops.label_vote_sweep(y, labels, lut, [], conf, 0)
  bad = lut.copy()
  bad[40] = 9
  for call in (lambda: ops.label_vote_sweep(y, labels, bad, [0.5], conf, 0), lambda: ops.label_planes(y, labels, bad, 0.5)):
    with pytest.raises(rn.RecAttendError, match=r'lut\[40\] = 9'):
      call()
  with pytest.raises(rn.RecAttendError, match='lut must be uint8'):
    ops.label_planes(y, labels, lut[:100], 0.5)
  with pytest.raises(rn.RecAttendError, match='labels .* do not belong to y'):
    ops.label_vote_sweep(y, z(1, 4, 5, dt=torch.uint8), lut, [0.5], conf, 0)
  with pytest.raises(rn.RecAttendError, match='labels must be a torch.uint8 tensor'):
    ops.label_planes(y, z(1, 4, 4, dt=torch.int32), lut, 0.5)
  with pytest.raises(rn.RecAttendError, match='y must be a torch.float32 tensor of 4'):
    ops.label_planes(z(2, 4, 4), labels, lut, 0.5)
  with pytest.raises(rn.RecAttendError, match='y must be contiguous'):
    ops.label_planes(z(1, 2, 4, 8)[..., ::2], labels, lut, 0.5)
  with pytest.raises(rn.RecAttendError, match='conf must be float32'):
    ops.label_vote_sweep(y, labels, lut, [0.5], z(1, 3), 0)
  with pytest.raises(rn.RecAttendError, match='keep must be uint8'):
    ops.label_planes(y, labels, lut, 0.5, keep=z(1, 2))
  with pytest.raises(rn.RecAttendError, match='remove_tiny'):
    ops.label_vote_sweep(y, labels, lut, [0.5], conf, 0.5)
  for host in ('y', 'labels', 'conf'):
    args = {'y': y, 'labels': labels, 'conf': conf}
    args[host] = args[host].cpu()
    with pytest.raises(rn.RecAttendError, match='%s must be a CUDA' % host):
      ops.label_vote_sweep(args['y'], args['labels'], lut, [0.5], args['conf'], 0)
  with pytest.raises(rn.RecAttendError, match='labels must be a CUDA'):
    ops.label_planes(y, labels.cpu(), lut, 0.5)
  with pytest.raises(rn.RecAttendError, match='keep must be a CUDA'):
    ops.label_planes(y, labels, lut, 0.5, keep=torch.ones(1, 2, dtype=torch.uint8))


def _tree(root):
  out = {}
  for folder, _, files in os.walk(root):
    for f in files:
      out[os.path.relpath(os.path.join(folder, f), root)] = open(os.path.join(folder, f), 'rb').read()
  return out


def test_command_line_end_to_end(cuda, tmp_path):
  """--semantic_labels DIR and --semantic_labels file.npz at 32 x 64: the .txt lines and the PNG bytes the oracle's text_lines
  and masks give, and with gt_instance_ids the AP json of CityscapesAPAnalyzer run on the oracle's masks."""
  import analysis
  import cityscapes_eval as ce
  from utils import png
  from utils import postprocess as pp
  ths, remove_tiny, H, W = [0.3, 0.0, 0.5], 30, 32, 64
  names = ['aachen_000001_000019', 'bonn_000002_000019', 'bonn_000003_000019']
  noise, labels, s = lo.scene(21, 3, 5, H // 2, W // 2, ths)
  rng = np.random.RandomState(4)
  y_ins = np.abs(noise) * np.float32(0.2)            # five bars on low noise, at network size 16 x 32
  for t in range(5):
    y_ins[:, t, 3:13, 1 + 6 * t:6 + 6 * t] = 0.95 - 0.1 * t
  s[:, 2:] = rng.uniform(0.7, 1.0, (3, 3)).astype(np.float32)
  labels = np.repeat(np.repeat(labels, 2, axis=1), 2, axis=2)
  gt_ids = labels.astype(np.int32)
  for b in range(3):
    for t in range(2, 5):                              # under three of the bars one thing class, and a ground-truth instance
      labels[b, 6:26, 2 + 12 * t:12 + 12 * t] = lo.LABEL_IDS[(b + t) % 8]
      gt_ids[b, 6:26, 2 + 12 * t:12 + 12 * t] = lo.LABEL_IDS[(b + t) % 8] * 1000 + t
  s[:, 0], s[:, 1] = 0.5, 0.2
  seg_dir = tmp_path / 'seg'
  for b, n in enumerate(names):
    (seg_dir / n.split('_')[0]).mkdir(parents=True, exist_ok=True)
    png.write_gray8(str(seg_dir / n.split('_')[0] / (n + '_pred_labelIds.png')), labels[b])
  seg_npz = str(tmp_path / 'seg.npz')
  np.savez(seg_npz, labels=labels[::-1], names=np.array(names[::-1]))
  src = str(tmp_path / 'in.npz')   # no y_out: the pre-stage's map is not needed
  np.savez(src, y_out_ins=y_ins, s_out=s, names=np.array(names), full_size=np.array([H, W]), gt_instance_ids=gt_ids)

  # the oracle on the masks the unchanged front of the chain hands over
  yd = pp.apply_confidence(pp.upsample(_dev(y_ins), (H, W)), _dev(s))[0]
  y = yd.cpu().numpy()
  lut = lo.class_lut('labelIds')
  ref = lo.sweep(y, labels, lut, ths, s, remove_tiny)
  masks = [lo.planes(y, labels, lut, th, ref['keep'][k]) for k, th in enumerate(ths)]
  assert (ref['class_idx'][-1] >= 0).sum() >= 3 and (ref['class_idx'][:, :, :2] == -1).all()

  common = ['--input', src, '--threshold_list', ','.join(str(t) for t in ths), '--remove_tiny', str(remove_tiny), '--batch_size',
            '2', '--analyzers', '']
  out_a, out_b = str(tmp_path / 'out_a'), str(tmp_path / 'out_b')
  renders = ce.main(common + ['--output', out_a, '--semantic_labels', str(seg_dir)])
  ce.main(common + ['--output', out_b, '--semantic_labels', seg_npz, '--semantic_label_ids', 'labelIds'])
  a, b = _tree(out_a), _tree(out_b)
  assert a == b                       # folder and .npz: the same files, byte for byte
  for k, r in enumerate(renders):     # every threshold's records
    got = {os.path.basename(fn): lines for fn, lines in r.written}
    for i, n in enumerate(names):
      assert got[n + '.txt'] == lo.text_lines(n, ref['conf'][k, i], ref['label_id'][k, i], ref['class_idx'][k, i])
  want = {}                           # what the last threshold leaves on disk (plus PNGs of earlier thresholds it did not rewrite)
  for i, n in enumerate(names):
    lines = lo.text_lines(n, ref['conf'][-1, i], ref['label_id'][-1, i], ref['class_idx'][-1, i])
    folder = os.path.join('output_valid', 'cityscapes', n.split('_')[0])
    want[os.path.join(folder, n + '.txt')] = ''.join(analysis.cityscapes_line(*l) for l in lines).encode()
    for t in np.flatnonzero(ref['class_idx'][-1, i] >= 0):
      want[os.path.join(folder, '%s_%03d.png' % (n, t))] = png.encode_gray8((masks[-1][i, t] * 255).astype(np.uint8))
  assert len(want) > 5 and all(a[k] == v for k, v in want.items())

  js = json.loads(a[os.path.join('output_valid', 'resultInstanceLevelSemanticLabeling.json')].decode())
  for k, th in enumerate(ths):
    scorer = analysis.CityscapesAPAnalyzer(names)
    scorer.stage({'y_out': _dev(masks[k]), 'gt_ids': _dev(gt_ids), 'label_id': ref['label_id'][k], 'conf': ref['conf'][k],
                  'indices': [0, 1, 2]})
    res = json.loads(json.dumps(scorer.finalize(quiet=True)))
    assert json.dumps(res['averages'], sort_keys=True) == json.dumps(js['thresholds']['%.2f' % th], sort_keys=True)
    if k == len(ths) - 1:
      assert json.dumps(res, sort_keys=True) == json.dumps({x: v for x, v in js.items() if x != 'thresholds'}, sort_keys=True)
  assert js['averages']['allAp50%'] > 0
