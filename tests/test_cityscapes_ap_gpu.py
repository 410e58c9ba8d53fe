"""The matching step of the Cityscapes instance-level AP on the MI355X: the ground-truth catalogue (ra_gt_instance_catalog_i32)
against np.unique and the overlap counts (ra_instance_overlap_f32) against np.bincount — integers, so everything is compared
for equality — then CityscapesAPAnalyzer end to end against the loop-by-loop oracle of tests/ap_oracle.py run on the FILES
the output stage wrote (1e-12 on every AP: float64 sums of a few thousand terms <= 1 on both sides), and the two command
lines."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import ap_oracle as ao
import ra_native as rn
import ra_ops as ops

pytestmark = pytest.mark.gpu
AP_TOL = 1e-12
G = 256


def _reference(gt, y):
  """Per image: (ids, pixels) = np.unique, inter [T, n] by np.bincount over the slots, pred_pixels [T]."""
  out = []
  for b in range(gt.shape[0]):
    ids, slot, pixels = np.unique(gt[b].ravel(), return_inverse=True, return_counts=True)
    nz = y[b].reshape(y.shape[1], -1) != 0
    inter = np.stack([np.bincount(slot[m], minlength=ids.size) for m in nz])
    out.append((ids, pixels, inter, nz.sum(axis=1)))
  return out


def _run(gt, y):
  gt_d, y_d = torch.from_numpy(gt).cuda(), torch.from_numpy(y).cuda()
  ids, pixels, count, status = ops.gt_instance_catalog(gt_d, check_status=False)
  inter, pred = ops.instance_overlap(y_d, gt_d, (ids, pixels, count))
  assert all(t.dtype == torch.int32 for t in (ids, pixels, count, status, inter, pred))
  assert tuple(ids.shape) == tuple(pixels.shape) == (gt.shape[0], G) and tuple(inter.shape) == y.shape[:2] + (G,)
  return [t.cpu().numpy() for t in (ids, pixels, count, status, inter, pred)]


def _check(gt, y, what):
  """Catalogue and counts of every image equal the reference's; returns the device results."""
  ids, pixels, count, status, inter, pred = got = _run(gt, y)
  for b, (r_ids, r_pix, r_inter, r_pred) in enumerate(_reference(gt, y)):
    n = r_ids.size
    assert status[b] == 0 and count[b] == n, (what, b, status[b], count[b], n)
    assert np.array_equal(ids[b, :n], r_ids) and np.array_equal(pixels[b, :n], r_pix), (what, b)
    assert (ids[b, n:] == -1).all() and (pixels[b, n:] == 0).all()
    assert np.array_equal(inter[b, :, :n], r_inter) and not inter[b, :, n:].any(), (what, b)
    assert np.array_equal(pred[b], r_pred), (what, b)
    assert np.array_equal(inter[b].sum(axis=1), pred[b])
  return got


def _blocks(rng, B, H, W, n_inst):
  """An instance-id image of rectangles: a few label ids below 1000 as ground, instances labelId * 1000 + k on top, with a
  different number of them in every image of the batch."""
  gt = np.zeros((B, H, W), np.int32)
  for b in range(B):
    gt[b] = rng.choice([0, 3, 7, 8, 11, 26])
    gt[b, H // 2:] = rng.choice([21, 23, 24])
    for k in range(n_inst + 3 * b):
      r0, c0 = rng.randint(0, H), rng.randint(0, W)
      r1, c1 = r0 + rng.randint(1, max(2, H // 3)), c0 + rng.randint(1, max(2, W // 3))
      gt[b, r0:r1, c0:c1] = rng.choice([24, 25, 26, 27, 28, 31, 32, 33]) * 1000 + k
  return gt


def _masks(rng, B, T, H, W, values=(1.0,)):
  """T rectangles per image, overlapping where they fall on each other, filled with the given non-zero values in turn."""
  y = np.zeros((B, T, H, W), np.float32)
  for b in range(B):
    for t in range(T):
      r0, c0 = rng.randint(0, H), rng.randint(0, W)
      y[b, t, r0:r0 + rng.randint(1, H), c0:c0 + rng.randint(1, W)] = values[t % len(values)]
  return y


# 37 x 53: odd width, H * W = 1961 is no multiple of 4 (element loads), two tiles of 1024 with a ragged second one
# 40 x 52: 16-byte loads;  50 x 90: 16-byte loads that cross row ends (W % 4 != 0, H * W % 4 == 0)
@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('T', [1, 5, 20, 32])
@pytest.mark.parametrize('shape', [(37, 53), (40, 52), (50, 90)], ids=['37x53', '40x52', '50x90'])
def test_catalogue_and_overlap_small(cuda, shape, T, B):
  rng = np.random.RandomState(1000 * B + 10 * T + shape[0])
  gt = _blocks(rng, B, shape[0], shape[1], 9)
  y = _masks(rng, B, T, shape[0], shape[1], values=(1.0, 0.5, -1.0, 255.0))
  got = _check(gt, y, (shape, T, B))
  assert got[5].max() > 0 and (B == 1 or len({int(c) for c in got[2]}) > 1)  # different catalogues in one batch
  again = _run(gt, y)
  assert all(np.array_equal(a, b) for a, b in zip(got, again))  # the same on every run


def test_single_id_whole_image_mask_empty_masks_and_overlaps(cuda):
  H, W = 37, 53
  gt = np.full((2, H, W), 26001, np.int32)
  gt[1, :, :20] = 65535                      # the largest id of a 16-bit image
  y = np.zeros((2, 4, H, W), np.float32)
  y[0, 0] = 1.0                              # one mask over the whole image on one id: every lane on one counter
  y[0, 1, 3:30, 5:50] = 0.5                  # overlapping the first, and each other
  y[0, 2, 10:37, 0:40] = -1.0
  y[1, 3, :, 10:30] = 1.0
  ids, pixels, count, status, inter, pred = _check(gt, y, 'single id')
  assert count.tolist() == [1, 2] and ids[1, :2].tolist() == [26001, 65535] and pixels[0, 0] == H * W
  assert inter[0, 0, 0] == H * W and pred[0].tolist() == [H * W, 27 * 45, 27 * 40, 0] and inter[1, 3, :2].tolist() == [10 * H, 10 * H]
  _, _, _, _, inter0, pred0 = _check(gt, np.zeros_like(y), 'all masks empty')
  assert not inter0.any() and not pred0.any()
  y[1, 2, 0, 0] = float('nan')               # a NaN is not zero, as in numpy
  _check(gt, y, 'nan')


def test_full_mask_on_one_id_at_16_byte_loads(cuda):
  gt = np.full((1, 64, 128), 7, np.int32)
  gt[0, :, 64:] = 24001
  y = np.ones((1, 32, 64, 128), np.float32)  # every mask covers everything
  _, _, count, _, inter, pred = _check(gt, y, 'all masks full')
  assert count[0] == 2 and (inter[0, :, :2] == 4096).all() and (pred == 8192).all()


def test_cap_of_256_ids_and_ids_out_of_range(cuda):
  H, W = 37, 53
  rng = np.random.RandomState(5)
  gt = _blocks(rng, 4, H, W, 6)
  gt[1].ravel()[:G] = 1000 + 7 * np.arange(G)            # image 1: exactly 256 distinct ids ...
  gt[1].ravel()[G:] = 1000
  gt[2].ravel()[:G + 1] = 40000 - 3 * np.arange(G + 1)   # image 2: 257
  gt[2].ravel()[G + 1:] = 40000
  y = _masks(rng, 4, 5, H, W)
  gt_d, y_d = torch.from_numpy(gt).cuda(), torch.from_numpy(y).cuda()
  ids, pixels, count, status = ops.gt_instance_catalog(gt_d, check_status=False)
  inter, pred = ops.instance_overlap(y_d, gt_d, (ids, pixels, count))
  torch.cuda.synchronize()                                # no fault
  ids, pixels, count, status, inter, pred = (t.cpu().numpy() for t in (ids, pixels, count, status, inter, pred))
  assert status.tolist() == [0, 0, rn.RA_GT_STATUS_COUNT, 0] and count.tolist()[1:3] == [G, G]
  ref = _reference(gt, y)
  for b in (0, 1, 3):                                     # the other images of the batch stay valid
    n = ref[b][0].size
    assert count[b] == n and np.array_equal(ids[b, :n], ref[b][0]) and np.array_equal(pixels[b, :n], ref[b][1])
    assert np.array_equal(inter[b, :, :n], ref[b][2]) and np.array_equal(pred[b], ref[b][3])
  assert np.array_equal(ids[2], ref[2][0][:G]) and np.array_equal(pixels[2], ref[2][1][:G])  # the 256 smallest of the 257
  assert np.array_equal(inter[2], ref[2][2][:, :G]) and np.array_equal(pred[2], ref[2][3])
  with pytest.raises(rn.RecAttendError, match='image 2 has more than 256 distinct instance ids'):
    ops.gt_instance_catalog(gt_d)
  with pytest.raises(rn.RecAttendError, match='image berlin_000002_000019 has more than 256'):
    ops.gt_instance_catalog(gt_d, names=['berlin_%06d_000019' % i for i in range(4)])
  # an id of 70000, and a negative one: an error that names the image, no fault, the other images valid
  gt[2] = 7
  gt[2, 3, 4:9] = 70000
  gt[3, 0, 0] = -5
  gt_d = torch.from_numpy(gt).cuda()
  ids, pixels, count, status = ops.gt_instance_catalog(gt_d, check_status=False)
  inter, pred = ops.instance_overlap(y_d, gt_d, (ids, pixels, count))
  torch.cuda.synchronize()
  ids, pixels, count, status, inter, pred = (t.cpu().numpy() for t in (ids, pixels, count, status, inter, pred))
  assert status.tolist() == [0, 0, rn.RA_GT_STATUS_RANGE, rn.RA_GT_STATUS_RANGE]
  assert count[2] == 1 and ids[2, 0] == 7 and pixels[2, 0] == H * W - 5
  ref = _reference(gt, y)
  for b in (0, 1):
    n = ref[b][0].size
    assert np.array_equal(ids[b, :n], ref[b][0]) and np.array_equal(inter[b, :, :n], ref[b][2])
  assert np.array_equal(pred[2], ref[2][3]) and np.array_equal(inter[2, :, 0], ref[2][2][:, 0])  # slot 0 is id 7 on both sides
  with pytest.raises(rn.RecAttendError, match='image 2 has an instance id outside'):
    ops.gt_instance_catalog(gt_d)


def test_more_ids_than_the_hash_tables_hold(cuda):
  """Above 512 distinct ids the 512-entry tables themselves fill up: in a workgroup's table (image 1: 600 ids within the first
  tile of 1024 pixels) and only in the merging table (image 2: 350 ids in each of the two tiles).  Which ids are kept then
  depends on arrival order, so only this is asserted: no fault, the status word, 256 distinct ids of the image in ascending
  order, counts that stay within the image, an error naming the first such image, and the other images unharmed."""
  H, W = 37, 53
  rng = np.random.RandomState(6)
  gt = _blocks(rng, 4, H, W, 6)
  gt[1].ravel()[:600] = 1000 + 11 * np.arange(600)
  gt[1].ravel()[600:] = 1000
  gt[2].ravel()[:350] = 2000 + 5 * np.arange(350)
  gt[2].ravel()[350:1024] = 2000
  gt[2].ravel()[1024:1374] = 30000 + 7 * np.arange(350)
  gt[2].ravel()[1374:] = 30000
  y = _masks(rng, 4, 5, H, W)
  gt_d, y_d = torch.from_numpy(gt).cuda(), torch.from_numpy(y).cuda()
  ids, pixels, count, status = ops.gt_instance_catalog(gt_d, check_status=False)
  inter, pred = ops.instance_overlap(y_d, gt_d, (ids, pixels, count))
  torch.cuda.synchronize()                                # no fault
  ids, pixels, count, status, inter, pred = (t.cpu().numpy() for t in (ids, pixels, count, status, inter, pred))
  assert status.tolist() == [0, rn.RA_GT_STATUS_COUNT, rn.RA_GT_STATUS_COUNT, 0] and count.tolist()[1:3] == [G, G]
  ref = _reference(gt, y)
  for b in (1, 2):
    assert (np.diff(ids[b]) > 0).all() and np.isin(ids[b], ref[b][0]).all()
    full = dict(zip(ref[b][0].tolist(), ref[b][1].tolist()))
    assert all(0 < p <= full[i] for i, p in zip(ids[b].tolist(), pixels[b].tolist()))
    assert np.array_equal(pred[b], ref[b][3]) and (inter[b] >= 0).all() and (inter[b].sum(axis=1) <= pred[b]).all()
  for b in (0, 3):
    n = ref[b][0].size
    assert status[b] == 0 and count[b] == n and np.array_equal(ids[b, :n], ref[b][0]) and np.array_equal(pixels[b, :n], ref[b][1])
    assert np.array_equal(inter[b, :, :n], ref[b][2]) and np.array_equal(pred[b], ref[b][3])
  with pytest.raises(rn.RecAttendError, match='image 1 has more than 256 distinct instance ids'):
    ops.gt_instance_catalog(gt_d)


@functools.lru_cache(maxsize=None)
def _full_size_case():
  rng = np.random.RandomState(20)
  H, W, T = 1024, 2048, 20
  gt = np.full((1, H, W), 7, np.int32)
  gt[0, :400] = 23
  gt[0, 1000:] = 1
  for k in range(60):
    r0, c0 = rng.randint(300, 950), rng.randint(0, 2000)
    gt[0, r0:r0 + rng.randint(20, 200), c0:c0 + rng.randint(20, 300)] = rng.choice([24, 25, 26, 27, 28, 33]) * 1000 + k
  y = np.zeros((1, T, H, W), np.float32)
  for t in range(T):
    r0, c0 = rng.randint(250, 900), rng.randint(0, 1900)
    y[0, t, r0:r0 + rng.randint(30, 250), c0:c0 + rng.randint(30, 400)] = 1.0
  y[0, 0] = 1.0  # and one mask over everything: 2^21 pixels, most of them on three counters
  return gt, y


def test_full_size(cuda):
  gt, y = _full_size_case()
  ids, pixels, count, status, inter, pred = _check(gt, y, '1024 x 2048')
  assert count[0] > 40 and pred[0, 0] == 1024 * 2048 and np.array_equal(inter[0, 0, :count[0]], pixels[0, :count[0]])


def test_wrapper_validation(cuda):
  gt = torch.zeros(1, 8, 8, dtype=torch.int32, device='cuda')
  cat = ops.gt_instance_catalog(gt)
  assert len(cat) == 3
  with pytest.raises(rn.RecAttendError, match='int32'):
    ops.gt_instance_catalog(gt.to(torch.int64))
  with pytest.raises(rn.RecAttendError, match='T=33'):
    ops.instance_overlap(torch.zeros(1, 33, 8, 8, device='cuda'), gt, cat)
  with pytest.raises(rn.RecAttendError, match='do not belong together'):
    ops.instance_overlap(torch.zeros(2, 3, 8, 8, device='cuda'), gt, cat)
  with pytest.raises(rn.RecAttendError, match='float32'):
    ops.instance_overlap(torch.zeros(1, 3, 8, 8, device='cuda', dtype=torch.float64), gt, cat)
  with pytest.raises(rn.RecAttendError, match='gt_ids must be contiguous, got strides'):
    ops.gt_instance_catalog(torch.zeros(1, 8, 16, dtype=torch.int32, device='cuda')[:, :, ::2])
  many = torch.zeros(65536, 1, 1, dtype=torch.int32, device='cuda')  # more images than the grid's second extent takes
  with pytest.raises(rn.RecAttendError, match='gt_instance_catalog: B=65536'):
    ops.gt_instance_catalog(many)
  cat_many = tuple(torch.zeros((65536,) + tuple(t.shape[1:]), dtype=torch.int32, device='cuda') for t in cat)
  with pytest.raises(rn.RecAttendError, match='instance_overlap: B=65536'):
    ops.instance_overlap(torch.zeros(65536, 1, 1, 1, device='cuda'), many, cat_many)


# ---- the analyzer and the command lines on the 96 x 160 scene
def _stage_inputs(sc):
  """The scene as the output stage's inputs: masks at network size 48 x 80 (2 x 2 block means), scores, and a semantic map
  that is background except under a prediction, where it is the prediction's class."""
  y = sc['y']
  B, T, H, W = y.shape
  y_ins = y.reshape(B, T, H // 2, 2, W // 2, 2).mean(axis=(3, 5)).astype(np.float32)
  s = np.where(sc['label_id'] >= 0, sc['conf'], 0.2).astype(np.float32)
  sem = np.zeros((B, H // 2, W // 2, 9), np.float32)
  sem[..., 0] = 1.0
  labels = [l for _, l in ao.INST_LABELS]
  for b in range(B):
    for t in range(T):
      if sc['label_id'][b, t] in labels:
        m = y_ins[b, t] > 0
        sem[b][m] = 0.0
        sem[b][m, 1 + labels.index(sc['label_id'][b, t])] = 1.0
  return y_ins, s, sem


def _nan_equal(a, b, tol):
  a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
  return np.array_equal(np.isnan(a), np.isnan(b)) and (np.nan_to_num(np.abs(a - b)) <= tol).all()


def test_analyzer_end_to_end_against_the_oracle_on_files(cuda, tmp_path):
  import analysis
  import cityscapes_eval as ce
  from utils import png
  sc = ao.scene(3)
  y_ins, s, sem = _stage_inputs(sc)
  H, W = sc['gt_ids'].shape[1:]
  gt_files = []
  for b, name in enumerate(sc['names']):  # the ground truth goes through a 16-bit PNG with Paeth rows
    f = tmp_path / ('%s_gtFine_instanceIds.png' % analysis._stem(name))
    f.write_bytes(ao.encode_gray16(sc['gt_ids'][b].astype(np.uint16), 4))
    gt_files.append(str(f))
  gt_read = np.stack([png.read_gray16(f).astype(np.int32) for f in gt_files])
  assert np.array_equal(gt_read, sc['gt_ids'])
  dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
  ths = [0.3, 0.5]
  n_lines = 0
  for tt, res in enumerate(ce.iter_label_instances(dev(y_ins), dev(s), dev(sem), (H, W), ths, remove_tiny=50)):
    res['indices'] = [0, 1, 2]
    render = analysis.RenderCityScapesOutputAnalyzer(str(tmp_path / ('th%d' % tt)), sc['names'])
    render.stage(res)
    scorer = analysis.CityscapesAPAnalyzer(sc['names'])
    res['gt_ids'] = dev(gt_read)
    scorer.stage(res)
    got = scorer.finalize(quiet=True)
    preds = [ao.read_result_files(text_fn, png.read_gray8) for text_fn, _ in render.written]
    n_lines += sum(len(p) for p in preds)
    ap_ref, avg_ref = ao.run(list(gt_read), preds)
    ap = np.array(got['resultApMatrix'])
    print('threshold %.1f: %d written instances, allAp %.6f (oracle %.6f), max |ap - oracle| = %.3g' % (
        ths[tt], sum(len(p) for p in preds), got['averages']['allAp'], avg_ref['allAp'], np.nanmax(np.abs(ap - ap_ref))))
    assert _nan_equal(ap, ap_ref, AP_TOL)
    assert abs(got['averages']['allAp'] - avg_ref['allAp']) <= AP_TOL and abs(got['averages']['allAp50%'] - avg_ref['allAp50%']) <= AP_TOL
    for name, _ in ao.INST_LABELS:
      for k in ('ap', 'ap50%'):
        assert _nan_equal(got['averages']['classes'][name][k], avg_ref['classes'][name][k], AP_TOL), (name, k)
    assert 0 < got['averages']['classes']['car']['ap50%'] <= 1 and np.isnan(got['averages']['classes']['bus']['ap'])
    # the scores of the records are the text files' (six decimals), not the float32 values
    written = sorted(c for p in preds for _, l, c in p)
    kept = sorted(c for _, r in scorer.records for c in r['pred_conf'].tolist())
    assert set(kept) <= set(written) and len(kept) >= 6
  assert n_lines >= 12
  assert any(float('%f' % c) != float(c) for c in sc['conf'].ravel() if c > 0)  # the rounding is not the identity on this scene


def test_analyzer_takes_more_than_32_predictions(cuda):
  """The kernel counts at most 32 predictions a launch; the analyzer splits a longer list.  70 masks (two full launches and
  a ragged third) give the match records of the counts made in NumPy, and the AP of those records."""
  import analysis
  rng = np.random.RandomState(8)
  B, T, H, W = 2, 70, 37, 53
  gt = _blocks(rng, B, H, W, 9)
  y = _masks(rng, B, T, H, W)
  lab = rng.choice([24, 26, 26, 26, 28, -1], size=(B, T)).astype(np.int32)
  conf = rng.rand(B, T).astype(np.float32)
  scorer = analysis.CityscapesAPAnalyzer(['a_000000_000000', 'a_000000_000001'])
  scorer.stage({'y_out': torch.from_numpy(y).cuda(), 'gt_ids': torch.from_numpy(gt).cuda(), 'label_id': lab, 'conf': conf,
                'indices': [0, 1]})
  want = [analysis.cityscapes_match_record(r_ids, r_pix, r_inter, r_pred, lab[b], conf[b])
          for b, (r_ids, r_pix, r_inter, r_pred) in enumerate(_reference(gt, y))]
  assert len(scorer.records) == B
  for (_, got), ref in zip(scorer.records, want):
    assert sorted(got) == sorted(ref) and got['inter'].shape[0] > 32
    for k in ref:
      assert np.array_equal(got[k], ref[k]), k
  assert _nan_equal(scorer.finalize(quiet=True)['resultApMatrix'], analysis.cityscapes_ap(want), 0)


def _tree(root):
  out = {}
  for folder, _, files in os.walk(root):
    for f in files:
      out[os.path.relpath(os.path.join(folder, f), root)] = open(os.path.join(folder, f), 'rb').read()
  return out


def test_command_lines(cuda, tmp_path):
  import cityscapes_ap as cap
  import cityscapes_eval as ce
  sc = ao.scene(3)
  y_ins, s, sem = _stage_inputs(sc)
  base = dict(y_out_ins=y_ins, s_out=s, y_out=sem, names=np.array(sc['names']), full_size=np.array([96, 160]))
  with_ids, without = str(tmp_path / 'a.npz'), str(tmp_path / 'b.npz')
  np.savez(with_ids, gt_instance_ids=sc['gt_ids'], **base)
  np.savez(without, **base)
  common = ['--threshold_list', '0.3,0.5', '--remove_tiny', '50', '--batch_size', '2', '--analyzers', '']
  out_a, out_b = str(tmp_path / 'out_a'), str(tmp_path / 'out_b')
  ce.main(['--input', with_ids, '--output', out_a] + common)
  ce.main(['--input', without, '--output', out_b] + common)
  a, b = _tree(out_a), _tree(out_b)
  js = os.path.join('output_valid', 'resultInstanceLevelSemanticLabeling.json')
  assert js in a and js not in b
  res = json.loads(a.pop(js).decode())
  assert a == b and len(a) > 8          # without the key nothing changes, byte for byte
  assert sorted(res) == ['averages', 'distanceThresholds', 'instLabels', 'minRegionSizes', 'minStereoDensities', 'overlaps',
                         'resultApMatrix', 'thresholds']
  assert sorted(res['thresholds']) == ['0.30', '0.50'] and _nan_equal(res['thresholds']['0.50']['allAp'], res['averages']['allAp'], 0)
  assert sorted(res['averages']) == ['allAp', 'allAp50%', 'classes'] and res['instLabels'] == [n for n, _ in ao.INST_LABELS]
  assert np.array(res['resultApMatrix']).shape == (1, 8, 10) and 0 < res['averages']['allAp50%'] <= 1
  # the files left on disk, scored by the stand-alone command line: the last threshold's numbers
  gt = str(tmp_path / 'gt.npz')
  np.savez(gt, gt_instance_ids=sc['gt_ids'], names=np.array(sc['names']))
  out_json = str(tmp_path / 'ap.json')
  got = cap.main(['--results', os.path.join(out_a, 'output_valid', 'cityscapes'), '--gt', gt, '--output', out_json, '--batch_size', '2'])
  assert _nan_equal(got['resultApMatrix'], res['resultApMatrix'], 0)
  assert got['averages']['allAp'] == res['averages']['allAp'] and got['averages']['allAp50%'] == res['averages']['allAp50%']
  assert _nan_equal(json.load(open(out_json))['resultApMatrix'], res['resultApMatrix'], 0)
  wrong = np.zeros((3, 48, 80), np.int32)
  np.savez(with_ids, gt_instance_ids=wrong, **base)
  with pytest.raises(rn.RecAttendError, match='gt_instance_ids'):
    ce.main(['--input', with_ids, '--output', str(tmp_path / 'out_c')] + common)
