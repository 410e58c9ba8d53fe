"""The Cityscapes instance-level AP without a GPU: the host part of analysis.CityscapesAPAnalyzer (match records -> AP)
against the loop-by-loop float64 oracle of tests/ap_oracle.py on a scene that takes every branch of the evaluation, the 16-bit
PNG reader on hand-filtered files, the refusals of cityscapes_ap.py, and the argument checks of the two entry points.

The AP bar, 1e-12 absolute: both sides sum at most a few thousand float64 terms of magnitude <= 1 (one ulp of 1 is 2.2e-16);
everything that is a count is compared for equality."""
import functools
import io
import os
import struct
import zlib

import numpy as np
import pytest

import ap_oracle as ao
import ra_native as rn

AP_TOL = 1e-12


def _records(sc):
  """Match records of a scene with the counts made in NumPy: np.unique for the catalogue, np.bincount for the overlaps."""
  import analysis
  out = []
  for b in range(sc['gt_ids'].shape[0]):
    gt = sc['gt_ids'][b].ravel()
    ids, slot, pixels = np.unique(gt, return_inverse=True, return_counts=True)
    T = sc['y'].shape[1]
    inter = np.stack([np.bincount(slot[sc['y'][b, t].ravel() != 0], minlength=ids.size) for t in range(T)])
    pred = (sc['y'][b].reshape(T, -1) != 0).sum(axis=1)
    out.append(analysis.cityscapes_match_record(ids, pixels, inter, pred, sc['label_id'][b], sc['conf'][b]))
  return out


@functools.lru_cache(maxsize=None)
def _scene_and_oracle(seed):
  sc = ao.scene(seed)
  ao.COUNTERS.clear()
  ap, avg = ao.run(list(sc['gt_ids']), ao.scene_preds(sc))
  return sc, ap, avg, dict(ao.COUNTERS)


def test_scene_takes_every_branch():
  sc, ap, avg, n = _scene_and_oracle(0)
  assert sc['gt_ids'].shape == (3, 96, 160) and (sc['gt_ids'][0] == 26).sum() == 1500          # a group of an evaluated class
  assert len(ao.BRANCHES) == 14
  for key in ao.BRANCHES:  # among them the 80-pixel person: covered, ignored ...
    assert n.get(key, 0) > 0, key
  person = [nm for nm, _ in ao.INST_LABELS].index('person')
  # ... and not a false positive: at overlap 0.5 the person class has the one false positive of image 1 only
  gts, preds = ao.assign(sc['gt_ids'][0], ao.scene_preds(sc)[0])
  assert [g['id'] for g in gts['person']] == [24001, 24002] and gts['person'][0]['pixels'] == 80
  assert preds['person'][0]['touching'][0]['inter'] == 80 and preds['person'][0]['pixels'] == 120
  truck = [nm for nm, _ in ao.INST_LABELS].index('truck')
  assert (ap[0, truck] == 0).all() and np.isnan(ap[0, 4:]).all() and np.isfinite(ap[0, :4]).all()
  # person: 24001 is too small to count, nobody finds 24002 (recall 0 at every score), and the examples are false positives
  # only (image 1's at every overlap, image 0's from 0.7 on, where 80 / 120 of it on the small person no longer excuse it):
  # tp = 0 throughout, so every recall step of the integration is 0 and the AP is exactly 0, not NaN
  assert (ap[0, person] == 0).all()
  car = 2
  assert 0 < ap[0, car, 0] < 1 and ap[0, car, 0] > ap[0, car, -1]
  assert sc['conf'][0, 0] == sc['conf'][0, 7] and sc['label_id'][0, 5] == -1 and not sc['y'][0, 6].any()
  assert 29001 in sc['gt_ids'][0] and ao.assign(sc['gt_ids'][0], [(sc['gt_ids'][0] == 29001, 26, 0.5)])[1]['car'][0]['void'] == 0


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_host_ap_matches_oracle(seed):
  import analysis
  sc, ap_ref, avg_ref, _ = _scene_and_oracle(seed)
  records = _records(sc)
  ap = analysis.cityscapes_ap(records)
  assert ap.shape == ap_ref.shape == (1, 8, 10) and ap.dtype == np.float64
  assert np.array_equal(np.isnan(ap), np.isnan(ap_ref))
  err = np.nanmax(np.abs(ap - ap_ref))
  print('seed %d: max |ap - oracle| = %.3g; car AP %s' % (seed, err, np.round(ap_ref[0, 2], 4).tolist()))
  assert err <= AP_TOL
  avg = analysis.cityscapes_ap_averages(ap)
  assert abs(avg['allAp'] - avg_ref['allAp']) <= AP_TOL and abs(avg['allAp50%'] - avg_ref['allAp50%']) <= AP_TOL
  for name, _ in ao.INST_LABELS:
    for k in ('ap', 'ap50%'):
      a, r = avg['classes'][name][k], float(avg_ref['classes'][name][k])
      assert (np.isnan(a) and np.isnan(r)) or abs(a - r) <= AP_TOL, (name, k)
  # the counts of the records are the oracle's
  for b, rec in enumerate(records):
    gts, preds = ao.assign(sc['gt_ids'][b], ao.scene_preds(sc)[b])
    kept = [p for name, _ in ao.INST_LABELS for p in preds[name]]
    assert sorted(rec['pred_pixels'].tolist()) == sorted(p['pixels'] for p in kept)
    assert sorted(rec['pred_void'].tolist()) == sorted(p['void'] for p in kept)
    assert sorted(rec['pred_conf'].tolist()) == sorted(p['conf'] for p in kept)
    want = {(g['id'], g['pixels']) for name, _ in ao.INST_LABELS for g in gts[name]}
    assert want <= set(zip(rec['gt_id'].tolist(), rec['gt_pixels'].tolist()))


def test_result_dict_table_and_json(tmp_path):
  import json
  import analysis
  sc, ap_ref, avg_ref, _ = _scene_and_oracle(0)
  an = analysis.CityscapesAPAnalyzer(sc['names'])
  an.records = list(zip(sc['names'], _records(sc)))
  path = str(tmp_path / 'r.json')
  res = an.finalize(path, quiet=True)
  assert sorted(res) == ['averages', 'distanceThresholds', 'instLabels', 'minRegionSizes', 'minStereoDensities', 'overlaps',
                         'resultApMatrix']  # prepareJSONDataForResults
  assert res['instLabels'] == [n for n, _ in ao.INST_LABELS] and res['minRegionSizes'] == [100, 1000, 1000]
  assert res['overlaps'] == ao.OVERLAPS.tolist() and res['distanceThresholds'] == [float('inf'), 100.0, 50.0]
  assert sorted(res['averages']) == ['allAp', 'allAp50%', 'classes'] and sorted(res['averages']['classes']['car']) == ['ap', 'ap50%']
  back = json.load(open(path))
  assert back['averages']['allAp'] == res['averages']['allAp'] and np.isnan(back['resultApMatrix'][0][7][0])
  table = analysis.cityscapes_ap_table(res['averages']).splitlines()
  assert table[1] == '#' * 50 and table[2] == 'what           :             AP         AP_50%' and '\x1b' not in ''.join(table)
  assert table[4].startswith('person         :') and table[-1].startswith('average        :') and table[-2] == '-' * 50
  assert table[6] == 'car            :%15.3f%15.3f' % (res['averages']['classes']['car']['ap'], res['averages']['classes']['car']['ap50%'])
  assert 'nan' in table[11]
  # the confidence is the text file's: six decimals
  rec = analysis.cityscapes_match_record([7, 26001], [50, 50], [[0, 30]], [40], [26], [np.float32(0.1234567)])
  assert rec['pred_conf'].tolist() == [0.123457] and rec['pred_void'].tolist() == [0]
  # void is a test on the raw value: 29 is void, 29001 is not
  rec = analysis.cityscapes_match_record([3, 29, 29001], [9, 9, 9], [[1, 2, 4]], [7], [24], [0.9])
  assert rec['pred_void'].tolist() == [3]


# ---- read_gray16
def _img16(shape, seed):
  rng = np.random.RandomState(seed)
  a = rng.randint(0, 65536, shape).astype(np.uint16)
  a[: shape[0] // 2] = 26001  # runs, as a real instance-id image has
  return a


@pytest.mark.parametrize('shape', [(1, 1), (1, 7), (5, 3), (37, 53)])
@pytest.mark.parametrize('filter_type', [0, 1, 2, 3, 4])
def test_read_gray16_every_filter(shape, filter_type, tmp_path):
  from utils import png
  img = _img16(shape, 10 * filter_type + shape[1])
  data = ao.encode_gray16(img, filter_type)
  raw = zlib.decompress([p for t, p, _ in png.iter_chunks(data) if t == b'IDAT'][0])
  assert set(raw[::2 * shape[1] + 1]) == {filter_type}  # the file really uses that filter on every row
  got = png.decode_gray16(data)
  assert got.dtype == np.uint16 and np.array_equal(got, img)
  (tmp_path / 'a.png').write_bytes(data)
  assert np.array_equal(png.read_gray16(str(tmp_path / 'a.png')), img)


def test_read_gray16_mixed_filters_and_split_idat():
  from utils import png
  img = _img16((10, 9), 3)
  H, W = img.shape
  raw = b''
  for r in range(H):  # row r filtered with type r % 5: take that row out of the file filtered with it throughout
    whole = zlib.decompress([p for t, p, _ in png.iter_chunks(ao.encode_gray16(img, r % 5)) if t == b'IDAT'][0])
    raw += whole[r * (2 * W + 1):(r + 1) * (2 * W + 1)]
  z = zlib.compress(raw)
  chunk = lambda tag, d: struct.pack('>I', len(d)) + tag + d + struct.pack('>I', zlib.crc32(tag + d) & 0xffffffff)
  data = (png.SIGNATURE + chunk(b'IHDR', struct.pack('>IIBBBBB', W, H, 16, 0, 0, 0, 0)) + chunk(b'tEXt', b'k\0v') +
          chunk(b'IDAT', z[:7]) + chunk(b'IDAT', z[7:]) + chunk(b'IEND', b''))
  assert np.array_equal(png.decode_gray16(data), img)


def test_read_gray16_refusals():
  from utils import png
  good = ao.encode_gray16(_img16((4, 4), 0), 4)
  bad = bytearray(good)
  bad[-20] ^= 1  # inside the IDAT payload
  with pytest.raises(ValueError, match='CRC'):
    png.decode_gray16(bytes(bad))
  with pytest.raises(ValueError, match='16-bit'):
    png.decode_gray16(png.encode_gray8(np.zeros((4, 4), np.uint8)))
  with pytest.raises(ValueError):
    png.decode_gray16(b'not a png')
  with pytest.raises(ValueError, match='filter type'):
    z = zlib.compress(b'\x07' + bytes(8))
    chunk = lambda tag, d: struct.pack('>I', len(d)) + tag + d + struct.pack('>I', zlib.crc32(tag + d) & 0xffffffff)
    png.decode_gray16(png.SIGNATURE + chunk(b'IHDR', struct.pack('>IIBBBBB', 4, 1, 16, 0, 0, 0, 0)) + chunk(b'IDAT', z) +
                      chunk(b'IEND', b''))
  with pytest.raises(ValueError, match='does not inflate'):  # image data cut short, the chunk itself in order
    png.decode_gray16(png.SIGNATURE + chunk(b'IHDR', struct.pack('>IIBBBBB', 4, 1, 16, 0, 0, 0, 0)) + chunk(b'IDAT', z[:-3]) +
                      chunk(b'IEND', b''))
  assert np.array_equal(png.decode_gray8(png.encode_gray8(np.arange(6, dtype=np.uint8).reshape(2, 3))),
                        np.arange(6, dtype=np.uint8).reshape(2, 3))  # the 8-bit functions are as they were


def test_read_gray16_file_written_by_pil():
  Image = pytest.importorskip('PIL.Image')
  from utils import png
  img = _img16((37, 53), 5)
  bio = io.BytesIO()
  Image.fromarray(img).save(bio, format='PNG')
  assert np.array_equal(png.decode_gray16(bio.getvalue()), img)


# ---- cityscapes_ap.py
def _write_tree(tmp_path, sc, which=(0, 1, 2)):
  """The scene as files: <results>/<run>/<name>.txt + masks, and the ground truth as gt.npz."""
  from utils import png
  import analysis
  res = tmp_path / 'results'
  for b in which:
    stem = analysis._stem(sc['names'][b])
    folder = res / stem.split('_')[0]
    folder.mkdir(parents=True, exist_ok=True)
    with open(str(folder / (stem + '.txt')), 'w') as f:
      for t in range(sc['y'].shape[1]):
        if sc['label_id'][b, t] < 0:
          continue
        name = '%s_%03d.png' % (stem, t)
        png.write_gray8(str(folder / name), (sc['y'][b, t] * 255).astype(np.uint8))
        f.write(analysis.cityscapes_line(name, sc['label_id'][b, t], sc['conf'][b, t]))
  gt = str(tmp_path / 'gt.npz')
  np.savez(gt, gt_instance_ids=sc['gt_ids'], names=np.array(sc['names']))
  return str(res), gt


def test_cityscapes_ap_refusals(tmp_path, monkeypatch):
  import torch
  import cityscapes_ap as cap
  sc = ao.scene(0)
  res, gt = _write_tree(tmp_path, sc, which=(0, 1))
  with pytest.raises(rn.RecAttendError, match='no prediction.*bochum_000001_000019'):
    cap.main(['--results', res, '--gt', gt])
  res, gt = _write_tree(tmp_path, sc)
  twin = os.path.join(res, 'aachen', 'aachen_000001_000019_again.txt')
  open(twin, 'w').close()
  with pytest.raises(rn.RecAttendError, match='multiple predictions.*aachen_000001_000019'):
    cap.main(['--results', res, '--gt', gt])
  os.remove(twin)
  txt = os.path.join(res, 'aachen', 'aachen_000001_000019.txt')
  keep = open(txt).read()
  open(txt, 'w').write(os.path.join(res, 'aachen', 'aachen_000001_000019_000.png') + ' 26 0.9\n')
  with pytest.raises(rn.RecAttendError, match='relative'):
    cap.main(['--results', res, '--gt', gt])
  open(txt, 'w').write('aachen_000001_000019_000.png 26\n')
  with pytest.raises(rn.RecAttendError, match='three fields'):
    cap.main(['--results', res, '--gt', gt])
  open(txt, 'w').write('../../gt.npz 26 0.9\n')
  with pytest.raises(rn.RecAttendError, match='outside'):
    cap.main(['--results', res, '--gt', gt])
  from utils import png
  png.write_gray8(os.path.join(res, 'aachen', 'small.png'), np.zeros((48, 80), np.uint8))
  open(txt, 'w').write('small.png 26 0.9\n')
  with pytest.raises(rn.RecAttendError, match='48 x 80.*96 x 160'):
    cap.main(['--results', res, '--gt', gt])
  open(txt, 'w').write(keep)
  monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
  with pytest.raises(rn.RecAttendError, match='no CPU fallback'):
    cap.main(['--results', res, '--gt', gt])
  assert cap.image_stem('/x/frankfurt_000001_000019_gtFine_instanceIds.png') == 'frankfurt_000001_000019'


def test_cityscapes_ap_reads_a_ground_truth_folder(tmp_path):
  import cityscapes_ap as cap
  sc = ao.scene(0)
  folder = tmp_path / 'gtFine' / 'val' / 'aachen'
  folder.mkdir(parents=True)
  (folder / 'aachen_000001_000019_gtFine_instanceIds.png').write_bytes(ao.encode_gray16(sc['gt_ids'][0].astype(np.uint16), 4))
  (folder / 'aachen_000001_000019_gtFine_labelIds.png').write_bytes(b'')
  (name, load), = cap.list_ground_truth(str(tmp_path / 'gtFine'))
  assert name.endswith('aachen_000001_000019_gtFine_instanceIds.png') and cap.image_stem(name) == 'aachen_000001_000019'
  got = load()
  assert got.dtype == np.int32 and np.array_equal(got, sc['gt_ids'][0])
  (tmp_path / 'nothing_here').mkdir()
  with pytest.raises(rn.RecAttendError, match='no .*_gtFine_instanceIds.png'):
    cap.list_ground_truth(str(tmp_path / 'nothing_here'))


# ---- no device, and the ABI
def test_no_device_raises(monkeypatch):
  import torch
  import ra_ops as ops
  monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
  gt = torch.zeros(1, 8, 8, dtype=torch.int32)
  with pytest.raises(rn.RecAttendError, match='no CPU fallback'):
    ops.gt_instance_catalog(gt)
  cat = (torch.zeros(1, ops.MAX_GT, dtype=torch.int32), torch.zeros(1, ops.MAX_GT, dtype=torch.int32), torch.zeros(1, dtype=torch.int32))
  with pytest.raises(rn.RecAttendError, match='no CPU fallback'):
    ops.instance_overlap(torch.zeros(1, 2, 8, 8), gt, cat)


def test_argument_validation_without_gpu():
  lib = rn.lib()
  assert rn.RA_OVERLAP_MAX_GT == 256 and (rn.RA_GT_STATUS_RANGE, rn.RA_GT_STATUS_COUNT) == (1, 2)
  for name in ('ra_gt_instance_catalog_i32', 'ra_gt_instance_catalog_workspace_ints', 'ra_instance_overlap_f32',
               'ra_instance_overlap_workspace_ints'):
    assert name in rn.SIGNATURES and hasattr(lib, name)
  one = 16  # any non-null address: the shape is refused before anything is read or launched
  big = 1 << 20
  assert lib.ra_instance_overlap_f32(one, one, one, one, 1, 33, 8, 8, one, big, one, one, None) == rn.RA_E_SHAPE
  assert b'T=33' in lib.ra_last_error_string()
  assert lib.ra_instance_overlap_f32(one, one, one, one, 1, 0, 8, 8, one, big, one, one, None) == rn.RA_E_SHAPE
  assert lib.ra_instance_overlap_f32(one, one, one, one, 1, 20, 32768, 65536, one, big, one, one, None) == rn.RA_E_SHAPE  # H * W = 2^31
  assert lib.ra_gt_instance_catalog_i32(one, 1, 65536, 32768, one, big, one, one, one, one, None) == rn.RA_E_SHAPE
  assert lib.ra_instance_overlap_f32(None, one, one, one, 1, 2, 8, 8, one, big, one, one, None) == rn.RA_E_INVALID
  assert lib.ra_gt_instance_catalog_i32(None, 1, 8, 8, one, big, one, one, one, one, None) == rn.RA_E_INVALID
  assert lib.ra_instance_overlap_f32(one, one, one, one, 1, 2, 8, 8, one, 3, one, one, None) == rn.RA_E_WORKSPACE
  assert lib.ra_gt_instance_catalog_i32(one, 1, 8, 8, one, 3, one, one, one, one, None) == rn.RA_E_WORKSPACE
  # workspaces: one record of 2 * 512 + 4 ints per catalogue workgroup (256 in all), T * 257 ints per overlap workgroup (1024 in all)
  assert lib.ra_gt_instance_catalog_workspace_ints(1, 1024, 2048) == 256 * 1028
  assert lib.ra_gt_instance_catalog_workspace_ints(3, 37, 53) == 3 * 2 * 1028
  assert lib.ra_instance_overlap_workspace_ints(1, 20, 1024, 2048) == 1024 * 20 * 257
  assert lib.ra_instance_overlap_workspace_ints(4, 20, 1024, 2048) == 4 * 256 * 20 * 257
  assert lib.ra_instance_overlap_workspace_ints(1, 33, 0, 8) == 0
