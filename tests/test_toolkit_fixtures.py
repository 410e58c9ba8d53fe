"""The float64 oracles of the Cityscapes stages and the host halves of the product against what the REFERENCE'S OWN PROGRAMS
computed: tests/golden/toolkit_{instance,pixel}.{npz,json} and toolkit_orientation.npz, recorded by oracle/toolkit_fixtures.py
from evalInstanceLevelSemanticLabeling.py, evalPixelLevelSemanticLabeling.py and data_api/orientation.py + sep_labels.py of
the reference (translated to Python 3, run unedited).  Until these fixtures the oracles were restatements by the author of
the kernels; a shared misreading would have passed every test.

Bars, none of them new: integers (confusion matrix, counts, classes, masks) equal; AP within AP_TOL = 1e-12 of
tests/test_cityscapes_ap_gpu.py with NaN in the same places; pixel scores under pixel_oracle.same_scores (1e-12 relative).
Orientation: equal wherever labels_oracle's pre-floor value is at least ORI_GUARD from an integer — on the ellipse images
that is every foreground pixel (asserted), on the hand-made edge masks at least 95 % of them and at least one pixel of every
mask (asserted).

With RECATTEND_REFERENCE=<checkout of the reference> the recipe is run again and has to give the committed files."""
import functools
import json
import os

import numpy as np
import pytest

import ap_oracle as ao
import labels_oracle as lo
import pixel_oracle as po
import toolkit_scenes as ts

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
AP_TOL = 1e-12  # tests/test_cityscapes_ap_gpu.py's (test_bars_are_the_projects_own holds it to that)
FILES = ('toolkit_instance.npz', 'toolkit_instance.json', 'toolkit_pixel.npz', 'toolkit_pixel.json', 'toolkit_orientation.npz')


@functools.lru_cache(maxsize=None)
def instance_fixture():
  with open(os.path.join(GOLDEN, 'toolkit_instance.json')) as f:
    recorded = json.load(f)
  npz = np.load(os.path.join(GOLDEN, 'toolkit_instance.npz'), allow_pickle=False)
  return ts.load_instance_scenes(npz), recorded['scenes'], ts.manifest_of(npz), recorded['manifest']


@functools.lru_cache(maxsize=None)
def pixel_fixture():
  with open(os.path.join(GOLDEN, 'toolkit_pixel.json')) as f:
    recorded = json.load(f)
  npz = np.load(os.path.join(GOLDEN, 'toolkit_pixel.npz'), allow_pickle=False)
  return ts.load_pixel_scenes(npz), recorded['scenes'], ts.manifest_of(npz), recorded['manifest']


@functools.lru_cache(maxsize=None)
def orientation_fixture():
  npz = np.load(os.path.join(GOLDEN, 'toolkit_orientation.npz'), allow_pickle=False)
  return {k: npz[k] for k in npz.files}, ts.manifest_of(npz)


def test_bars_are_the_projects_own():
  import test_cityscapes_ap
  import test_cityscapes_ap_gpu
  import test_labels_gpu
  assert AP_TOL == test_cityscapes_ap_gpu.AP_TOL == test_cityscapes_ap.AP_TOL and ts.ORI_GUARD == test_labels_gpu.ORI_GUARD
  assert ts.EDGE_EXCLUDED_CAP == 0.05


def test_fixtures_hold_what_they_should():
  scenes, recorded, man, man_json = instance_fixture()
  assert man == man_json and sorted(scenes) == sorted(recorded) == sorted(ts.INSTANCE_SCENES)
  assert sum(1 for n, s in ts.INSTANCE_SCENES.items() if s[0] == 'random' and s[2:5] == (3, 96, 160)) >= 4
  assert scenes['odd37x53']['gt_ids'].shape[1:] == (37, 53) and (scenes['many40']['label_id'] >= 0).sum(axis=1).max() == 40
  for name, sc in scenes.items():
    assert max(sc['gt_ids'].shape[1:]) <= 160 and (name == 'legacy0' or ts.confidences_distinct(sc)), name
  ao.COUNTERS.clear()
  for sc in scenes.values():
    ao.run(list(sc['gt_ids']), ao.scene_preds(sc))
  assert not [k for k in ao.BRANCHES if not ao.COUNTERS.get(k)]
  # what the issue lists for the random scenes, in every one of them
  for name, sc in scenes.items():
    if name == 'legacy0':
      continue
    gt, lab = sc['gt_ids'], sc['label_id']
    assert ((gt >= 24) & (gt < 34) & (gt != 29) & (gt != 30)).any() and np.isin(gt, ao.VOID_IDS).any() and (gt // 1000 >= 29).any() and (gt // 1000 <= 30).any()
    pix = (sc['y'] != 0).sum(axis=(2, 3))
    assert ((pix == 0) & (lab >= 0)).any() and ((pix > 0) & (pix < 100)).any() and np.isin(lab, [7, 29, 30]).any()
    last = gt[-1]
    assert any(l in lab[-1] and not (last // 1000 == l).any() for l in ts.EVALUATED)  # predicted, and no instance in that image
  pscenes, precorded, pman, pman_json = pixel_fixture()
  assert pman == pman_json and sorted(pscenes) == sorted(precorded) == sorted(ts.PIXEL_SCENES)
  assert not pscenes['special48x80'][0][1].any() and (pscenes['special48x80'][2][2] == 26007).sum() == 1 and not pscenes['zero37x53'][0].any()
  arrays, oman = orientation_fixture()
  for m in (man, pman, oman):
    assert sorted(m) == ['numpy', 'pillow', 'reference_sha256', 'seeds'] and len(m['reference_sha256']) == 9
    assert all(len(v) == 64 for v in m['reference_sha256'].values())
  for f in FILES:
    assert os.path.getsize(os.path.join(GOLDEN, f)) < 100 * 1024, f


def test_generators_reproduce_the_committed_inputs():
  scenes, _, man, _ = instance_fixture()
  for name, sc in scenes.items():
    again = ts.instance_scene(name, man['seeds'][name])
    for k in ('gt_ids', 'y', 'label_id', 'conf'):
      assert again[k].dtype == sc[k].dtype and again[k].tobytes() == sc[k].tobytes(), (name, k)
    assert again['names'] == sc['names']
  pscenes, _, pman, _ = pixel_fixture()
  for name, (pred, labels, ids, _) in pscenes.items():
    again = ts.pixel_scene(name, pman['seeds'][name])
    assert all(np.array_equal(a, b) and a.shape == b.shape for a, b in zip(again, (pred, labels, ids))), name
  arrays, oman = orientation_fixture()
  for name in ts.ORIENTATION_SCENES:
    again = ts.orientation_scene(name, oman['seeds'][name])
    assert again.dtype == np.uint8 and again.tobytes() == arrays[name + '/ids'].tobytes(), name


# ---- instance level
@pytest.mark.parametrize('name', sorted(ts.INSTANCE_SCENES))
def test_ap_oracle_equals_the_toolkit(name):
  scenes, recorded, _, _ = instance_fixture()
  sc = scenes[name]
  ap, avg = ao.run(list(sc['gt_ids']), ao.scene_preds(sc))
  got = {'resultApMatrix': ap.tolist(), 'averages': avg}
  worst = ts.assert_ap_result(got, recorded[name], AP_TOL, name)
  print('%s: allAp %.15f (toolkit %.15f), worst |oracle - toolkit| %.3g' % (name, avg['allAp'], recorded[name]['averages']['allAp'], worst))


@pytest.mark.parametrize('name', sorted(ts.INSTANCE_SCENES))
def test_host_ap_equals_the_toolkit(name, tmp_path):
  import analysis
  from test_cityscapes_ap import _records
  scenes, recorded, _, _ = instance_fixture()
  sc = scenes[name]
  an = analysis.CityscapesAPAnalyzer(sc['names'])
  an.records = list(zip(sc['names'], _records(sc)))
  path = str(tmp_path / 'r.json')
  got = an.finalize(path, quiet=True)
  assert sorted(got) == sorted(recorded[name])  # the product writes the toolkit's keys, all of them
  worst = ts.assert_ap_result(got, recorded[name], AP_TOL, name)
  with open(path) as f:
    ts.assert_ap_result(json.load(f), recorded[name], AP_TOL, name + ' (file)')
  print('%s: worst |host - toolkit| %.3g' % (name, worst))


def test_the_scenes_differ_in_their_ap():
  _, recorded, _, _ = instance_fixture()
  assert len({round(r['averages']['allAp'], 6) for r in recorded.values()}) == len(recorded)


# ---- pixel level
@pytest.mark.parametrize('name', sorted(ts.PIXEL_SCENES))
def test_pixel_oracle_equals_the_toolkit(name):
  scenes, recorded, _, _ = pixel_fixture()
  pred, labels, ids, _ = scenes[name]
  state, sc = po.evaluate(list(pred), list(labels), list(ids))
  assert state['conf'].tolist() == recorded[name]['confMatrix']
  po.same_scores(sc, recorded[name], rel=1e-12)
  worst = ts.assert_pixel_result(dict(sc, confMatrix=state['conf'].tolist(), labels=recorded[name]['labels'], priors=recorded[name]['priors']),
                                 recorded[name], name)
  print('%s: worst relative |oracle - toolkit| over the scores %.3g' % (name, worst))
  if name.startswith('zero'):
    assert all(v == 0.0 or np.isnan(v) for v in recorded[name]['classScores'].values()) and recorded[name]['averageScoreClasses'] == 0.0


@pytest.mark.parametrize('name', sorted(ts.PIXEL_SCENES))
def test_host_pixel_scores_equal_the_toolkit(name):
  import analysis
  scenes, recorded, _, _ = pixel_fixture()
  pred, labels, ids, _ = scenes[name]
  conf = np.zeros((34, 34), np.int64)
  np.add.at(conf, (labels.ravel().astype(int), pred.ravel().astype(int)), 1)
  stats = analysis.pixel_instance_stats()
  for b in range(pred.shape[0]):  # per image: the catalogue and the counts per slot, made in NumPy
    rows = po.instance_counts(pred[b], ids[b])
    analysis.pixel_instance_stats_add(stats, *[[r[k] for r in rows] for k in range(4)])
  got = analysis.cityscapes_pixel_result(conf, stats)
  assert set(recorded[name]) <= set(got) and set(got) - set(recorded[name]) == {'averageScorePredictedClasses'}
  worst = ts.assert_pixel_result(got, recorded[name], name)
  print('%s: worst relative |host - toolkit| over scores and priors %.3g' % (name, worst))


# ---- orientation
def _masks_of(arrays, key):
  return ts.unpack_masks(arrays[key + 'masks_packed'], tuple(arrays[key + 'masks_shape']), np.uint8)


@pytest.mark.parametrize('name', sorted(ts.ORIENTATION_SCENES))
def test_labels_oracle_equals_the_reference(name):
  arrays, _ = orientation_fixture()
  imgs = arrays[name + '/ids']
  total = excluded = 0
  for b, img in enumerate(imgs):
    key = '%s/%d/' % (name, b)
    masks, colours = lo.separate_labels(img)
    want = _masks_of(arrays, key)
    assert np.array_equal(np.stack(masks), want) and colours == arrays[key + 'colours'].tolist() and want.dtype == masks[0].dtype
    margin, cls = ts.orientation_margin(img)
    ref = arrays[key + 'class']
    assert cls.dtype == ref.dtype == np.uint8 and cls.shape == ref.shape
    fg = img > 0
    sure = margin >= ts.ORI_GUARD
    assert not ref[~fg].any() and np.array_equal(cls[~fg], ref[~fg])
    if name == 'edges':
      assert all((sure & (img == i)).any() for i in ts.EDGE_IDS)
    else:
      assert sure[fg].all()  # a condition on the input
    total, excluded = total + int(fg.sum()), excluded + int((fg & ~sure).sum())
    bad = int((cls != ref)[fg & sure].sum())
    print('%s image %d: %d foreground pixels, %d inside the guard, %d differ outside it, %d inside; classes %s' % (
        name, b, fg.sum(), (fg & ~sure).sum(), bad, (cls != ref)[fg & ~sure].sum(), np.unique(ref[fg]).tolist()))
    assert bad == 0
    # the 'one_hot' encoding of the reference is the class of the covering instance, and nothing on the background
    one_hot = arrays[key + 'one_hot']
    assert one_hot.shape == ref.shape + (8,) and np.array_equal(one_hot, (ref[..., None] == np.arange(8)) * fg[..., None])
  assert excluded <= ts.EDGE_EXCLUDED_CAP * total
  if name != 'edges':
    assert len(np.unique(np.concatenate([arrays['%s/%d/class' % (name, b)][imgs[b] > 0] for b in range(len(imgs))]))) == 8


def test_edge_masks_sit_where_the_small_terms_decide():
  """The centroid of every edge mask is one of its pixels: there the offset from the centroid is a few 1e-8 (the + 1e-7 of the
  pixel count moves the centroid) and the class comes from the reference's + 1e-8 and its strict > 0 tests alone."""
  img = ts.edge_masks()[0]
  for i, (r, c) in {1: (2, 29), 2: (5, 9), 3: (13, 25), 4: (13, 9), 5: (0, 0)}.items():
    rr, cc = np.nonzero(img == i)
    assert rr.mean() == r and cc.mean() == c and img[r, c] == i
  assert (img == 2).sum() == 13 and (img == 3).sum() == 11 and (img == 4).sum() == 49


# ---- the recipe
def test_recipe_gives_the_committed_fixtures(tmp_path):
  ref = os.environ.get('RECATTEND_REFERENCE')
  if not ref:
    pytest.skip('RECATTEND_REFERENCE is not set: needs a checkout of the reference to run its programs again')
  import toolkit_fixtures
  toolkit_fixtures.main(['--reference', ref, '--out', str(tmp_path)])
  for f in FILES:
    if f.endswith('.json'):
      assert (tmp_path / f).read_bytes() == open(os.path.join(GOLDEN, f), 'rb').read(), f
      continue
    new, old = np.load(str(tmp_path / f), allow_pickle=False), np.load(os.path.join(GOLDEN, f), allow_pickle=False)
    assert sorted(new.files) == sorted(old.files), f
    for k in old.files:
      assert new[k].dtype == old[k].dtype and new[k].shape == old[k].shape and new[k].tobytes() == old[k].tobytes(), (f, k)
    assert ts.manifest_of(new)['reference_sha256'] == ts.manifest_of(old)['reference_sha256']
    assert (tmp_path / f).read_bytes() == open(os.path.join(GOLDEN, f), 'rb').read(), f  # same libraries: the same bytes
