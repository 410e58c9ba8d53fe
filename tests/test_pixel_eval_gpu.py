"""The Cityscapes pixel-level evaluation on the MI355X: ops.pixel_confusion in its label form against the NumPy oracle
(tests/pixel_oracle.py) — integers, so equal —, ops.sem_labels against the float64 arg-max of the resized map outside a band
of 1e-5 around ties, the fused form against the label form, the status words, and fg_model_eval end to end.

The arg-max band: float32 evaluates a resized value to a few 1e-7, so a pixel whose two largest float64 values differ by at
least 1e-5 has one answer; pixels inside the band are left out and must be at most 0.1 % of the image (a condition on the
inputs, asserted: smooth_semantic_map with bg_bias = 0.0, seeds 0 .. 4, puts 5e-5 of the pixels there at the first shape, none at the second)."""
import functools
import json
import math
import os

import numpy as np
import pytest
import torch

import cs_oracle as cso
import fg_model
import fg_model_eval
import fg_oracle as fo
import pixel_oracle as po
import ra_native as rn
import ra_ops as ops

pytestmark = pytest.mark.gpu
GAP = 1e-5
BAND_SHARE = 1e-3
TILE = ops.PIXEL_TILE
# 37 x 53: odd sizes, element loads, two tiles; the second: 16-byte loads, three workgroups per image, the last tile partly filled
SHAPES = [(2, 37, 53), (2, (2 * TILE + TILE // 2) // 64 + 1, 64)]


def _dev(a, dtype):
  return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


@functools.lru_cache(maxsize=None)
def _scene(shape, seed=0):
  B, H, W = shape
  rng = np.random.RandomState(100 + seed + H)
  pred, labels, ids = (np.stack(a) for a in zip(*[po.random_scene(rng, H, W) for _ in range(B)]))
  return pred, labels, ids


def _expected(pred, labels, ids):
  """(conf [34,34], inst_tp [B,256], inst_cat_tp [B,256], state) of the oracle; slots beyond an image's ids are 0."""
  state = po.new_state()
  B = pred.shape[0]
  tp, ctp = np.zeros((B, ops.MAX_GT), np.int64), np.zeros((B, ops.MAX_GT), np.int64)
  for b in range(B):
    po.evaluate_pair(pred[b], labels[b], ids[b], state)
    rows = po.instance_counts(pred[b], ids[b])
    tp[b, :len(rows)] = [r[2] for r in rows]
    ctp[b, :len(rows)] = [r[3] for r in rows]
  return state['conf'], tp, ctp, state


def _check(out, want, what):
  conf, tp, ctp = want[:3]
  got = out['conf'].cpu().numpy()
  assert got.dtype == np.int64 and (got == conf).all(), (what, np.argwhere(got != conf)[:5])
  assert (out['inst_tp'].cpu().numpy() == tp).all(), what
  assert (out['inst_cat_tp'].cpu().numpy() == ctp).all(), what


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%dx%d' % s)
@pytest.mark.parametrize('derived', [False, True], ids=['gt_labels', 'labels_from_ids'])
def test_label_form_equals_the_oracle(cuda, shape, derived):
  B, H, W = shape
  pred, labels, ids = _scene(shape)
  for a in (pred, labels):
    assert all(len(np.unique(a[b])) == 34 for b in range(B))  # every label occurs in ground truth and prediction
  assert (po.labels_of_ids(ids) == labels).all()
  ntiles = -(-H * W // TILE)
  assert ntiles >= (3 if H * W % 4 == 0 else 2) and H * W % TILE != 0 and ntiles <= 1024 // B  # one workgroup per tile
  want = _expected(pred, labels, ids)
  out = ops.pixel_confusion(_dev(pred, np.uint8), _dev(ids, np.int32), None if derived else _dev(labels, np.uint8))
  _check(out, want, shape)
  assert int(out['conf'].sum()) == B * H * W  # the toolkit's sanity check
  cat_ids, cat_pix, cat_n = (t.cpu().numpy() for t in out['catalog'])
  for b in range(B):
    rows = po.instance_counts(pred[b], ids[b])
    assert cat_n[b] == len(rows) and [(r[0], r[1]) for r in rows] == list(zip(cat_ids[b, :len(rows)], cat_pix[b, :len(rows)]))
  again = ops.pixel_confusion(_dev(pred, np.uint8), _dev(ids, np.int32), _dev(labels, np.uint8), catalog=out['catalog'])
  _check(again, want, 'with the catalogue handed in')


def test_catalogue_edge_256_ids(cuda):
  H, W = 48, 64  # three tiles; flat index 1024 is (16, 0)
  ids = np.repeat(np.arange(24), 2)[:, None].repeat(W, axis=1)  # 24 bare labels, bands of two rows
  ids[0, 10:13] = 1000
  things = [24, 25, 26, 27, 28, 29, 30, 31, 32, 33]  # 29, 30: instances of ignored labels
  for k in range(231):
    r, c = (k // 16) * 3 + 1, (k % 16) * 4
    ids[r, c:c + (1 if k == 0 else 2)] = things[k % 10] * 1000 + k  # k = 0: one pixel
  ids[15:17, 2:4] = things[1] * 1000 + 1  # instance 1 also lies on both sides of the boundary between tiles 0 and 1
  assert len(np.unique(ids)) == ops.MAX_GT and (ids == 29005).any() and (ids == things[0] * 1000).sum() == 1
  labels = po.labels_of_ids(ids)
  rng = np.random.RandomState(3)
  pred = labels.copy()
  for _ in range(30):
    r, c = rng.randint(0, H - 4), rng.randint(0, W - 8)
    pred[r:r + 4, c:c + 8] = rng.randint(0, 34)
  want = _expected(pred[None], labels[None], ids[None])
  for gl in (None, _dev(labels[None], np.uint8)):
    out = ops.pixel_confusion(_dev(pred[None], np.uint8), _dev(ids[None], np.int32), gl)
    assert int(out['catalog'][2][0]) == ops.MAX_GT
    _check(out, want, '256 ids')
  with pytest.raises(rn.RecAttendError, match='more than 256'):
    ids2 = ids.copy()
    ids2[47, 63] = 33999
    ops.pixel_confusion(_dev(pred[None], np.uint8), _dev(ids2[None], np.int32), names=['x.png'])


def test_accumulation_into_int64(cuda):
  a, b = _scene(SHAPES[0]), _scene(SHAPES[0], seed=1)
  start = (np.arange(34 * 34, dtype=np.int64).reshape(34, 34) * 7919) + (1 << 33)  # beyond 32 bits from the start
  conf = _dev(start, np.int64)
  wa, wb = _expected(*a), _expected(*b)
  out = ops.pixel_confusion(_dev(a[0], np.uint8), _dev(a[2], np.int32), _dev(a[1], np.uint8), conf=conf)
  assert out['conf'] is conf
  out = ops.pixel_confusion(_dev(b[0], np.uint8), _dev(b[2], np.int32), _dev(b[1], np.uint8), conf=conf)
  assert (conf.cpu().numpy() == start + wa[0] + wb[0]).all()
  assert (out['inst_tp'].cpu().numpy() == wb[1]).all()  # per call, not accumulated
  both = _expected(*[np.concatenate([x, y]) for x, y in zip(a, b)])
  assert (both[0] == wa[0] + wb[0]).all()
  # the same bits on every run
  runs = [ops.pixel_confusion(_dev(a[0], np.uint8), _dev(a[2], np.int32))['conf'].cpu().numpy() for _ in range(3)]
  assert (runs[0] == runs[1]).all() and (runs[0] == runs[2]).all()


ARGMAX_SHAPES = [(24, 40, 96, 160), (37, 53, 100, 131)]


@functools.lru_cache(maxsize=None)
def _sem_case(shape):
  """Seeds 0 .. 4, one image each: (sem float32 [5,Hs,Ws,9], float64 full-size map, its arg-max labels, outside-the-band mask)."""
  Hs, Ws, H, W = shape
  sem = np.concatenate([cso.smooth_semantic_map(np.random.RandomState(seed), 1, Hs, Ws, 9, bg_bias=0.0) for seed in range(5)])
  full = cso.sem_full(sem, H, W)
  return sem, full, po.argmax_labels(full), po.top2_gap(full) >= GAP


@pytest.mark.parametrize('shape', ARGMAX_SHAPES, ids=lambda s: '%dx%d-%dx%d' % s)
def test_sem_labels_equal_the_float64_argmax_outside_the_band(cuda, shape):
  Hs, Ws, H, W = shape
  sem, full, want, sure = _sem_case(shape)
  share = 1.0 - sure.mean()
  print('pixels inside the band: %d of %d (%.5f %%)' % ((~sure).sum(), sure.size, 100 * share))
  assert share <= BAND_SHARE
  assert sorted(np.unique(want)) == [0] + po.THING_LABELS  # all nine classes occur
  got = ops.sem_labels(_dev(sem, np.float32), (H, W))
  assert got.dtype == torch.uint8 and tuple(got.shape) == (5, H, W)
  got = got.cpu().numpy()
  print('pixels that differ outside the band: %d; inside: %d' % ((got != want)[sure].sum(), (got != want)[~sure].sum()))
  assert (got[sure] == want[sure]).all()


def test_sem_labels_ties_go_to_the_lower_channel(cuda):
  rng = np.random.RandomState(8)
  sem = rng.rand(2, 24, 40, 9).astype(np.float32) * 0.5
  sem[0, ..., 3] = sem[0, ..., 5] = sem[0].max(axis=-1) + rng.rand(24, 40).astype(np.float32)  # equal at every tap
  sem[1, ..., 0] = sem[1, ..., 4] = sem[1].max(axis=-1) + rng.rand(24, 40).astype(np.float32)
  for size in ((96, 160), (61, 103)):
    got = ops.sem_labels(_dev(sem, np.float32), size).cpu().numpy()
    assert (got[0] == po.THING_LABELS[2]).all() and (got[1] == 0).all()
  two = ops.sem_labels(_dev(sem[..., :2], np.float32), (30, 50)).cpu().numpy()  # C = 2: background or person
  assert set(np.unique(two)) == {0, 24}


@pytest.mark.parametrize('shape', ARGMAX_SHAPES, ids=lambda s: '%dx%d-%dx%d' % s)
@pytest.mark.parametrize('derived', [False, True], ids=['gt_labels', 'labels_from_ids'])
def test_fused_form_equals_the_label_form(cuda, shape, derived):
  Hs, Ws, H, W = shape
  sem = _dev(_sem_case(shape)[0][:2], np.float32)
  _, labels, ids = _scene((2, H, W))
  ids_d, gl = _dev(ids, np.int32), None if derived else _dev(labels, np.uint8)
  lab = ops.sem_labels(sem, (H, W))
  a = ops.pixel_confusion(lab, ids_d, gl)
  b = ops.pixel_confusion(sem, ids_d, gl, size=(H, W))
  for k in ('conf', 'inst_tp', 'inst_cat_tp'):
    assert torch.equal(a[k], b[k]), k
  _check(a, _expected(lab.cpu().numpy(), labels, ids), 'label form on the device labels')  # and that one is pinned to the oracle


def test_status_names_the_image_and_spares_the_others(cuda):
  B, H, W = 3, 37, 53
  pred, labels, ids = (np.stack([a[0], a[1], a[0]]) for a in _scene((2, H, W)))
  pred, labels, ids = pred.copy(), labels.copy(), ids.copy()
  pred[1, 5, 7] = 34
  pred[1, 30, 2:9] = 255
  labels[2, 11, 13:17] = 40
  names = ['a.png', 'b.png', 'c.png']
  args = (_dev(pred, np.uint8), _dev(ids, np.int32), _dev(labels, np.uint8))
  with pytest.raises(rn.RecAttendError, match=r'image b\.png has a predicted label above 33'):
    ops.pixel_confusion(*args, names=names)
  ok = torch.tensor([True, False, True])
  with pytest.raises(rn.RecAttendError, match=r'image 1 has a ground-truth label above 33'):
    ops.pixel_confusion(args[0][ok], args[1][ok], args[2][ok].contiguous())
  raw = ops.pixel_confusion(*args, names=names, check_status=False)
  assert raw['status'].cpu().tolist() == [0, rn.RA_PIXEL_STATUS_PRED, rn.RA_PIXEL_STATUS_GT]
  # pixels with a label above 33 are in no cell; everything else is counted as usual
  valid = (pred < 34) & (labels < 34)
  conf = np.zeros((34, 34), np.int64)
  np.add.at(conf, (labels[valid].astype(int), pred[valid].astype(int)), 1)
  assert (raw['conf'].cpu().numpy() == conf).all() and conf.sum() == B * H * W - 8 - 4
  clean = _expected(pred[:1], labels[:1], ids[:1])
  assert (raw['inst_tp'].cpu().numpy()[0] == clean[1][0]).all() and (raw['inst_cat_tp'].cpu().numpy()[0] == clean[2][0]).all()
  for b in (1, 2):  # the instance counts do not look at gt_labels, and a label above 33 matches no instance
    rows = po.instance_counts(pred[b], ids[b])
    assert raw['inst_tp'].cpu().numpy()[b, :len(rows)].tolist() == [r[2] for r in rows]
  # derived labels: an id whose label is above 33
  ids2 = ids.copy()
  ids2[0, 3, 3] = 40000
  with pytest.raises(rn.RecAttendError, match=r'image a\.png has a ground-truth label above 33'):
    ops.pixel_confusion(_dev(np.minimum(pred, 33), np.uint8), _dev(ids2, np.int32), names=names)


def test_command_line_end_to_end(cuda, tmp_path, capsys):
  import yaml
  opt = dict(fo.reduced_opt(9, False), segm_loss_fn='bce')
  P = fo.random_weights(opt, 71)
  res = str(tmp_path / 'results')
  os.makedirs(os.path.join(res, 'fg'))
  with open(os.path.join(res, 'fg', 'model_opt.yaml'), 'w') as f:
    yaml.safe_dump(opt, f)
  np.savez(os.path.join(res, 'fg', 'weights.npz'), step=np.float32(1), **P)
  rng = np.random.RandomState(72)
  N, h, w, H, W = 3, 32, 48, 61, 103
  x = rng.rand(N, h, w, 3).astype(np.float32)
  _, labels, ids = (np.stack(a) for a in zip(*[po.random_scene(rng, H, W) for _ in range(N)]))
  fg = (ids >= 1000).astype(np.uint8)
  names = np.array(['a.png', 'b.png', 'c.png'])
  plain, with_ids, with_both = (str(tmp_path / n) for n in ('plain.npz', 'ids.npz', 'both.npz'))
  np.savez(plain, x=x, fg_gt_full=fg, names=names)
  np.savez(with_ids, x=x, fg_gt_full=fg, names=names, gt_instance_ids=ids)
  np.savez(with_both, x=x, fg_gt_full=fg, names=names, gt_instance_ids=ids, gt_label_ids=labels)
  outs = {}
  for key, src in (('plain', plain), ('ids', with_ids), ('both', with_both)):
    o = str(tmp_path / ('out_' + key))
    fg_model_eval.main(['--model_id', 'fg', '--results', res, '--input', src, '--output', o, '--batch_size', '2'])
    with open(os.path.join(o, 'metrics.yaml')) as f:
      outs[key] = (o, yaml.safe_load(f))
  # without the keys: no file, no entry; with them: everything else as before
  assert sorted(outs['plain'][1]) == ['0.30'] and not os.path.exists(os.path.join(outs['plain'][0], 'resultPixelLevelSemanticLabeling.json'))
  for key in ('ids', 'both'):
    assert sorted(outs[key][1]) == ['0.30', 'pixel_level'] and outs[key][1]['0.30'] == outs['plain'][1]['0.30']
  # the oracle on the device's own arg-max labels, batch by batch as the script runs the net
  m = fg_model.get_model(opt).load_weights(P)
  dev_labels = np.concatenate([ops.sem_labels(m.run('y_out', {'x': _dev(x[b0:b0 + 2], np.float32), 'phase_train': False}).contiguous(),
                                              (H, W)).cpu().numpy() for b0 in (0, 2)])
  assert len(np.unique(dev_labels)) > 1
  _, want = po.evaluate(list(dev_labels), list(labels), list(ids))
  for key in ('ids', 'both'):
    with open(os.path.join(outs[key][0], 'resultPixelLevelSemanticLabeling.json')) as f:
      disk = json.load(f)
    po.same_scores(disk, want, rel=1e-12)
    state = po.new_state()
    for b in range(N):
      po.evaluate_pair(dev_labels[b], labels[b], ids[b], state)
    assert disk['confMatrix'] == state['conf'].tolist()
    px = outs[key][1]['pixel_level']
    assert sorted(px) == sorted(po.AVERAGE_KEYS + ['averageScorePredictedClasses'])
    for k in po.AVERAGE_KEYS:
      assert (math.isnan(px[k]) and math.isnan(want[k])) or abs(px[k] - want[k]) <= 1e-12 * abs(want[k])
  assert 'classes          IoU      nIoU' in capsys.readouterr().out
  # a model with several classes but not nine says why it leaves the scores out
  opt3 = dict(fo.reduced_opt(3, False), segm_loss_fn='bce')
  os.makedirs(os.path.join(res, 'fg3'))
  with open(os.path.join(res, 'fg3', 'model_opt.yaml'), 'w') as f:
    yaml.safe_dump(opt3, f)
  np.savez(os.path.join(res, 'fg3', 'weights.npz'), step=np.float32(1), **fo.random_weights(opt3, 73))
  o3 = str(tmp_path / 'out_3')
  fg_model_eval.main(['--model_id', 'fg3', '--results', res, '--input', with_ids, '--output', o3, '--batch_size', '2'])
  assert 'the model has 3 semantic classes' in capsys.readouterr().out
  assert not os.path.exists(os.path.join(o3, 'resultPixelLevelSemanticLabeling.json'))


def test_pixel_command_line(cuda, tmp_path):
  import cityscapes_pixel
  pred, labels, ids = _scene(SHAPES[0])
  gdir, pdir = tmp_path / 'gt' / 'ulm', tmp_path / 'pred'
  os.makedirs(str(gdir))
  os.makedirs(str(pdir))
  for b in range(2):
    stem = 'ulm_00000%d_000019' % b
    (gdir / (stem + '_gtFine_labelIds.png')).write_bytes(po.encode_png(labels[b], 8))
    (gdir / (stem + '_gtFine_instanceIds.png')).write_bytes(po.encode_png(ids[b], 16))
    (pdir / (stem + '_pred.png')).write_bytes(po.encode_png(pred[b], 8))
  out = str(tmp_path / 'result.json')
  res = cityscapes_pixel.main(['--pred', str(pdir), '--gt', str(tmp_path / 'gt'), '--output', out, '--batch_size', '1'])
  state, want = po.evaluate(list(pred), list(labels), list(ids))
  po.same_scores(res, want, rel=1e-12)
  assert res['confMatrix'] == state['conf'].tolist()
  with open(out) as f:
    po.same_scores(json.load(f), want, rel=1e-12)
  npz = str(tmp_path / 'gt.npz')
  np.savez(npz, gt_instance_ids=ids, names=np.array(['ulm_00000%d_000019.png' % b for b in range(2)]))
  po.same_scores(cityscapes_pixel.main(['--pred', str(pdir), '--gt', npz, '--output', out]), want, rel=1e-12)
