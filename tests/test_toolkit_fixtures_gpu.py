"""The device stages of the Cityscapes evaluation against what the REFERENCE'S OWN PROGRAMS computed (tests/golden/toolkit_*,
recorded by oracle/toolkit_fixtures.py; tests/test_toolkit_fixtures.py says what the files hold and holds the oracles and the
host halves to them): CityscapesAPAnalyzer and cityscapes_ap.py, ops.pixel_confusion / CityscapesPixelAnalyzer and
cityscapes_pixel.py, and the orientation classes of ops.assemble_labels.  Nothing but tests/golden/ is read.

The bars are those of the older tests: counts and the 34 x 34 matrix equal; AP within AP_TOL = 1e-12 with NaN in the same
places; pixel scores under pixel_oracle.same_scores (1e-12 relative); orientation classes equal wherever labels_oracle's
pre-floor value lies at least ORI_GUARD from an integer, which on the ellipse images is every foreground pixel (asserted)."""
import json
import os

import numpy as np
import pytest
import torch

import ap_oracle as ao
import pixel_oracle as po
import ra_ops as ops
import toolkit_scenes as ts
from test_cityscapes_ap import _records
from test_cityscapes_ap_gpu import AP_TOL
from test_labels_gpu import ORI_GUARD
from test_toolkit_fixtures import instance_fixture, orientation_fixture, pixel_fixture

pytestmark = pytest.mark.gpu


def _dev(a, dtype):
  return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


# ---- instance level
@pytest.mark.parametrize('name', sorted(ts.INSTANCE_SCENES))
def test_analyzer_equals_the_toolkit(cuda, name):
  import analysis
  scenes, recorded, _, _ = instance_fixture()
  sc = scenes[name]
  B, T = sc['y'].shape[:2]
  if name == 'many40':
    assert T > ops.OVERLAP_MAX_T  # two launches of the overlap kernel
  if name == 'odd37x53':
    assert sc['y'].shape[2] * sc['y'].shape[3] % 4 != 0
  scorer = analysis.CityscapesAPAnalyzer(sc['names'])
  scorer.stage({'y_out': _dev(sc['y'], np.float32), 'gt_ids': _dev(sc['gt_ids'], np.int32), 'label_id': sc['label_id'],
                'conf': sc['conf'], 'indices': list(range(B))})
  for (_, got), ref in zip(scorer.records, _records(sc)):  # the counts of the kernels are NumPy's
    assert sorted(got) == sorted(ref)
    for k in ref:
      assert np.array_equal(got[k], ref[k]), (name, k)
  got = scorer.finalize(quiet=True)
  assert sorted(got) == sorted(recorded[name])
  worst = ts.assert_ap_result(got, recorded[name], AP_TOL, name)
  print('%s: allAp %.15f (toolkit %.15f), worst |device - toolkit| %.3g' % (
      name, got['averages']['allAp'], recorded[name]['averages']['allAp'], worst))


@pytest.mark.parametrize('name', sorted(ts.INSTANCE_SCENES))
def test_cityscapes_ap_command_line_equals_the_toolkit(cuda, name, tmp_path):
  """The file route: text files and 8-bit masks below --results, the ground truth as 16-bit PNG files (read_gray16)."""
  import analysis
  import cityscapes_ap as cap
  from utils import png
  scenes, recorded, _, _ = instance_fixture()
  sc = scenes[name]
  res, gt_dir = tmp_path / 'results', tmp_path / 'gtFine' / 'val' / 'x'
  gt_dir.mkdir(parents=True)
  for b, img_name in enumerate(sc['names']):
    stem = analysis._stem(img_name)
    (gt_dir / (stem + '_gtFine_instanceIds.png')).write_bytes(ao.encode_gray16(sc['gt_ids'][b].astype(np.uint16), b % 5))
    folder = res / stem.split('_')[0]
    folder.mkdir(parents=True, exist_ok=True)
    with open(str(folder / (stem + '.txt')), 'w') as f:
      for t in range(sc['y'].shape[1]):
        if sc['label_id'][b, t] < 0:
          continue
        mask = '%s_%03d.png' % (stem, t)
        png.write_gray8(str(folder / mask), (sc['y'][b, t] * 255).astype(np.uint8))
        f.write(analysis.cityscapes_line(mask, sc['label_id'][b, t], sc['conf'][b, t]))
  out = str(tmp_path / 'ap.json')
  got = cap.main(['--results', str(res), '--gt', str(tmp_path / 'gtFine'), '--output', out, '--batch_size', '2'])
  worst = ts.assert_ap_result(got, recorded[name], AP_TOL, name)
  with open(out) as f:
    ts.assert_ap_result(json.load(f), recorded[name], AP_TOL, name + ' (file)')
  print('%s: worst |command line - toolkit| %.3g' % (name, worst))


# ---- pixel level
@pytest.mark.parametrize('name', sorted(ts.PIXEL_SCENES))
@pytest.mark.parametrize('derived', [False, True], ids=['gt_labels', 'labels_from_ids'])
def test_pixel_confusion_and_analyzer_equal_the_toolkit(cuda, name, derived):
  import analysis
  scenes, recorded, _, _ = pixel_fixture()
  pred, labels, ids, names = scenes[name]
  out = ops.pixel_confusion(_dev(pred, np.uint8), _dev(ids, np.int32), None if derived else _dev(labels, np.uint8))
  conf = out['conf'].cpu().numpy()
  assert conf.dtype == np.int64 and conf.tolist() == recorded[name]['confMatrix']
  scorer = analysis.CityscapesPixelAnalyzer(names)
  res = {'pred': _dev(pred, np.uint8), 'gt_ids': _dev(ids, np.int32), 'indices': list(range(len(names)))}
  if not derived:
    res['gt_labels'] = _dev(labels, np.uint8)
  scorer.stage(res)
  got = scorer.finalize(quiet=True)
  assert set(recorded[name]) <= set(got)
  worst = ts.assert_pixel_result(got, recorded[name], name)
  print('%s: averageScoreClasses %.15f (toolkit %.15f), averageScoreInstClasses %.15f (toolkit %.15f), worst relative |device - toolkit| %.3g' % (
      name, got['averageScoreClasses'], recorded[name]['averageScoreClasses'], got['averageScoreInstClasses'],
      recorded[name]['averageScoreInstClasses'], worst))


@pytest.mark.parametrize('name', sorted(ts.PIXEL_SCENES))
def test_cityscapes_pixel_command_line_equals_the_toolkit(cuda, name, tmp_path):
  import cityscapes_pixel
  scenes, recorded, _, _ = pixel_fixture()
  pred, labels, ids, names = scenes[name]
  gdir, pdir = tmp_path / 'gt' / 'x', tmp_path / 'pred'
  os.makedirs(str(gdir))
  os.makedirs(str(pdir))
  for b, stem in enumerate(names):
    (gdir / (stem + '_gtFine_labelIds.png')).write_bytes(po.encode_png(labels[b], 8))
    (gdir / (stem + '_gtFine_instanceIds.png')).write_bytes(po.encode_png(ids[b], 16))
    (pdir / (stem + '_pred.png')).write_bytes(po.encode_png(pred[b], 8))
  out = str(tmp_path / 'result.json')
  got = cityscapes_pixel.main(['--pred', str(pdir), '--gt', str(tmp_path / 'gt'), '--output', out, '--batch_size', '2'])
  ts.assert_pixel_result(got, recorded[name], name)
  with open(out) as f:
    ts.assert_pixel_result(json.load(f), recorded[name], name + ' (file)')


# ---- orientation
@pytest.mark.parametrize('name', sorted(ts.ORIENTATION_SCENES))
def test_orientation_classes_equal_the_reference(cuda, name):
  arrays, _ = orientation_fixture()
  imgs = arrays[name + '/ids']
  B, H, W = imgs.shape
  got = ops.assemble_labels(_dev(imgs, np.int32), H, W, 8, 'cvppp', want=('d_cls', 'd_gt'))  # the native size: no resize
  d_cls, d_gt = got['d_cls'].cpu().numpy(), got['d_gt'].cpu().numpy()
  total = excluded = 0
  for b, img in enumerate(imgs):
    ref = arrays['%s/%d/class' % (name, b)]
    margin, _ = ts.orientation_margin(img)
    fg = img > 0
    sure = margin >= ORI_GUARD
    if name == 'edges':
      assert all((sure & (img == i)).any() for i in ts.EDGE_IDS)
    else:
      assert sure[fg].all()  # a condition on the input
    total, excluded = total + int(fg.sum()), excluded + int((fg & ~sure).sum())
    compare = sure | ~fg
    bad = int((d_cls[b] != ref)[compare].sum())
    print('%s image %d: %d foreground pixels, %d inside the guard, %d differ outside it' % (name, b, fg.sum(), (fg & ~sure).sum(), bad))
    assert bad == 0, (name, b, np.argwhere((d_cls[b] != ref) & compare)[:5].tolist())
    assert np.array_equal(d_gt[b][compare], (ref[..., None] == np.arange(8)).astype(np.float32)[compare])
  assert excluded <= ts.EDGE_EXCLUDED_CAP * total
