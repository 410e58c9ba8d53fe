#!/usr/bin/env python
"""Records what the reference's own Cityscapes programs compute on the scenes of tests/toolkit_scenes.py, as the fixtures
tests/golden/toolkit_{instance,pixel}.{npz,json} and toolkit_orientation.npz (test infrastructure; the product never imports
this).

  python oracle/toolkit_fixtures.py --reference DIR [--out tests/golden]

DIR is a checkout of the reference.  Its evaluation scripts (instance level, pixel level, with the modules they import) and
data_api/orientation.py + sep_labels.py are Python 2.  The recipe copies them to oracle/_ref/toolkit/ (kept out of git),
translates the copies with lib2to3 and runs them as they are; four settings are made from outside, by assignment:

  PIL.PILLOW_VERSION            the helper module refuses to load without it; today's Pillow calls it __version__;
  np.float, np.bool, np.int     aliases that NumPy has dropped;
  args.predictionPath           the folder of the prediction files (the scripts otherwise look at environment variables);
  np.expand_dims                while get_orientation runs: the axis clamped to ndim — old NumPy accepted axis > ndim and
                                appended the axis, which is what that function relies on.

Every scene runs in a temporary working directory (the instance evaluator writes matches.json to the current one), and the
evaluator's gtInstances.json cache, which lies beside the translated script and is reused silently for other ground truth, is
deleted before every scene.  The .npz files hold the inputs (prediction masks bit-packed); the .json files hold, per scene,
the result file the toolkit wrote, parsed and gathered, NaN as NaN.  Every fixture carries a manifest: the sha256 of every
reference file that was translated, the NumPy and Pillow versions and the seeds.  The files are written with fixed zip
time stamps, so the same reference and the same libraries give the same bytes.

Conditions on the scenes, asserted here before anything is written: confidences pairwise distinct within a class after the
'%f' rounding (the toolkit sorts with NumPy's default argsort, which is not stable beyond 16 elements; only the hand-placed
scene legacy0 keeps its one deliberate tie, which is a tie of a true and a false example and lands in one threshold whatever
the order); the scenes together take every branch ap_oracle.BRANCHES lists; on the hand-made orientation masks at most 5 % of
the foreground lies within ORI_GUARD of a class boundary and every mask keeps a compared pixel."""
import argparse
import hashlib
import importlib
import io
import json
import os
import shutil
import subprocess
import sys
import tempfile
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_DIR = os.path.join(ROOT, 'oracle', '_ref', 'toolkit')
TOOLKIT = 'data_api/cityscapes_scripts'
FILES = [TOOLKIT + '/evaluation/evalInstanceLevelSemanticLabeling.py', TOOLKIT + '/evaluation/evalPixelLevelSemanticLabeling.py',
         TOOLKIT + '/evaluation/instances2dict.py', TOOLKIT + '/evaluation/instance.py', TOOLKIT + '/helpers/csHelpers.py',
         TOOLKIT + '/helpers/labels.py', TOOLKIT + '/helpers/annotation.py', 'data_api/orientation.py', 'data_api/sep_labels.py']


def translate(reference):
  """Copies FILES to REF_DIR, translates the copies -> {file: sha256 of the original}."""
  if os.path.isdir(REF_DIR):
    shutil.rmtree(REF_DIR)
  digests = {}
  for rel in FILES:
    src, dst = os.path.join(reference, rel), os.path.join(REF_DIR, rel)
    os.makedirs(os.path.dirname(dst), exist_ok=True)
    with open(src, 'rb') as f:
      digests[rel] = hashlib.sha256(f.read()).hexdigest()
    shutil.copyfile(src, dst)
  subprocess.check_call([sys.executable, '-W', 'ignore', '-m', 'lib2to3', '-w', '-n', REF_DIR], stdout=subprocess.DEVNULL,
                        stderr=subprocess.DEVNULL)
  return digests


def load_modules():
  import PIL
  PIL.PILLOW_VERSION = PIL.__version__
  np.float, np.bool, np.int = float, bool, int
  for sub in (TOOLKIT + '/evaluation', TOOLKIT + '/helpers', 'data_api'):
    sys.path.insert(0, os.path.join(REF_DIR, sub))
  names = ('evalInstanceLevelSemanticLabeling', 'evalPixelLevelSemanticLabeling', 'orientation', 'sep_labels')
  return [importlib.import_module(n) for n in names]


def _call(fn, *args):
  try:
    return fn(*args)
  except SystemExit:
    raise RuntimeError('the toolkit gave up (its message is above)')


def _save_png(path, img):
  from PIL import Image
  Image.fromarray(np.ascontiguousarray(img)).save(path, format='PNG')


def _stem(name):
  return name[:-4] if name.endswith('.png') else name


def run_instance(mod, sc):
  """One scene through evalInstanceLevelSemanticLabeling.evaluateImgLists -> the parsed result file."""
  if os.path.exists(mod.args.gtInstancesFile):
    os.remove(mod.args.gtInstancesFile)
  keep = os.getcwd()
  with tempfile.TemporaryDirectory() as tmp:
    gt_dir, res_dir = os.path.join(tmp, 'gt'), os.path.join(tmp, 'results')
    os.makedirs(gt_dir)
    os.makedirs(res_dir)
    gts, preds = [], []
    for b, name in enumerate(sc['names']):
      stem = _stem(name)
      gts.append(os.path.join(gt_dir, stem + '_gtFine_instanceIds.png'))
      _save_png(gts[-1], sc['gt_ids'][b].astype(np.uint16))
      preds.append(os.path.join(res_dir, stem + '.txt'))
      with open(preds[-1], 'w') as f:
        for t in range(sc['y'].shape[1]):
          if sc['label_id'][b, t] < 0:
            continue
          mask = '%s_%03d.png' % (stem, t)
          _save_png(os.path.join(res_dir, mask), ((sc['y'][b, t] != 0) * 255).astype(np.uint8))
          f.write('%s %d %f\n' % (mask, int(sc['label_id'][b, t]), float(sc['conf'][b, t])))
    a = mod.args
    a.predictionPath, a.predictionWalk = os.path.abspath(res_dir), None
    a.exportFile = os.path.join(tmp, 'out', 'resultInstanceLevelSemanticLabeling.json')
    a.quiet, a.colorized = True, False
    os.chdir(tmp)
    try:
      _call(mod.evaluateImgLists, preds, gts, a)
    finally:
      os.chdir(keep)
      if os.path.exists(a.gtInstancesFile):
        os.remove(a.gtInstancesFile)
    with open(a.exportFile) as f:
      return json.load(f)


def run_pixel(mod, scene, names):
  pred, labels, ids = scene
  keep = os.getcwd()
  with tempfile.TemporaryDirectory() as tmp:
    gt_dir, pred_dir = os.path.join(tmp, 'gt'), os.path.join(tmp, 'pred')
    os.makedirs(gt_dir)
    os.makedirs(pred_dir)
    gts, preds = [], []
    for b, stem in enumerate(names):
      gts.append(os.path.join(gt_dir, stem + '_gtFine_labelIds.png'))
      _save_png(gts[-1], labels[b].astype(np.uint8))
      _save_png(os.path.join(gt_dir, stem + '_gtFine_instanceIds.png'), ids[b].astype(np.uint16))
      preds.append(os.path.join(pred_dir, stem + '_pred.png'))
      _save_png(preds[-1], pred[b].astype(np.uint8))
    a = mod.args
    a.predictionPath, a.predictionWalk = os.path.abspath(pred_dir), None
    a.exportFile = os.path.join(tmp, 'out', 'resultSemanticLabeling.json')
    a.quiet = True
    os.chdir(tmp)
    try:
      _call(mod.evaluateImgLists, preds, gts, a)
    finally:
      os.chdir(keep)
    with open(a.exportFile) as f:
      return json.load(f)


def run_orientation(ori, sep, img):
  """One id image uint8 [H,W] -> (class [H,W], one_hot [H,W,8], masks [T,H,W], colours [T])."""
  masks, colours = sep.get_separate_labels(img)
  y = np.stack(masks)[None].astype(np.float64)
  real = np.expand_dims
  np.expand_dims = lambda a, axis: real(a, min(axis, np.ndim(a)) if axis >= 0 else axis)
  try:
    cls = ori.get_orientation(y, encoding='class')[0]
    one_hot = ori.get_orientation(y, encoding='one_hot')[0]
  finally:
    np.expand_dims = real
  return cls, one_hot, np.stack(masks), np.array(colours, np.uint64)


def write_npz(path, arrays):
  """np.savez_compressed with a fixed member order and fixed time stamps."""
  with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED) as z:
    for key in sorted(arrays):
      buf = io.BytesIO()
      np.lib.format.write_array(buf, np.asanyarray(arrays[key]), allow_pickle=False)
      info = zipfile.ZipInfo(key + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
      info.compress_type, info.external_attr = zipfile.ZIP_DEFLATED, 0o644 << 16
      z.writestr(info, buf.getvalue())


def write_json(path, manifest, per_scene):
  with open(path, 'w') as f:
    json.dump({'manifest': manifest, 'scenes': per_scene}, f, indent=1, sort_keys=True)
    f.write('\n')


def main(argv=None):
  p = argparse.ArgumentParser(description=__doc__.split('\n')[0])
  p.add_argument('--reference', required=True, help='a checkout of the reference')
  p.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden'))
  args = p.parse_args(argv)
  sys.path.insert(0, os.path.join(ROOT, 'tests'))
  digests = translate(os.path.abspath(args.reference))
  keep_path = list(sys.path)
  try:
    inst_mod, pix_mod, ori_mod, sep_mod = load_modules()
    record(args.out, digests, inst_mod, pix_mod, ori_mod, sep_mod)
  finally:  # the settings go with the run
    sys.path[:] = keep_path
    for alias in ('float', 'bool', 'int'):
      if alias in vars(np):
        delattr(np, alias)


def record(out, digests, inst_mod, pix_mod, ori_mod, sep_mod):
  import ap_oracle as ao
  import toolkit_scenes as ts
  import PIL
  os.makedirs(out, exist_ok=True)

  def manifest(table):
    return {'reference_sha256': digests, 'numpy': np.__version__, 'pillow': PIL.__version__,
            'seeds': {name: spec[1] if isinstance(spec[0], str) else spec[0] for name, spec in table.items()}}

  # ---- instance level
  scenes = {name: ts.instance_scene(name) for name in ts.INSTANCE_SCENES}
  ao.COUNTERS.clear()
  for name, sc in scenes.items():
    assert name == 'legacy0' or ts.confidences_distinct(sc), '%s: equal confidences within a class' % name
    assert (sc['label_id'] >= 0).sum(axis=1).max() > (32 if name == 'many40' else 0)
    ao.run(list(sc['gt_ids']), ao.scene_preds(sc))  # also: no class without any example, on which the toolkit fails
  missing = [k for k in ao.BRANCHES if not ao.COUNTERS.get(k)]
  assert not missing, 'branches no scene takes: %s' % missing
  results = {name: run_instance(inst_mod, sc) for name, sc in scenes.items()}
  man = manifest(ts.INSTANCE_SCENES)
  write_npz(os.path.join(out, 'toolkit_instance.npz'), dict(ts.instance_arrays(scenes), manifest=np.array(json.dumps(man, sort_keys=True))))
  write_json(os.path.join(out, 'toolkit_instance.json'), man, results)

  # ---- pixel level
  scenes = {name: ts.pixel_scene(name) for name in ts.PIXEL_SCENES}
  arrays = ts.pixel_arrays(scenes)
  results = {name: run_pixel(pix_mod, sc, [str(n) for n in arrays[name + '/names']]) for name, sc in scenes.items()}
  man = manifest(ts.PIXEL_SCENES)
  write_npz(os.path.join(out, 'toolkit_pixel.npz'), dict(arrays, manifest=np.array(json.dumps(man, sort_keys=True))))
  write_json(os.path.join(out, 'toolkit_pixel.json'), man, results)

  # ---- orientation
  man = manifest(ts.ORIENTATION_SCENES)
  arrays = {'scenes': np.array(sorted(ts.ORIENTATION_SCENES)), 'manifest': np.array(json.dumps(man, sort_keys=True))}
  for name in ts.ORIENTATION_SCENES:
    imgs = ts.orientation_scene(name)
    arrays[name + '/ids'] = imgs
    for b, img in enumerate(imgs):
      cls, one_hot, masks, colours = run_orientation(ori_mod, sep_mod, img)
      margin, _ = ts.orientation_margin(img)
      fg = img > 0
      if name == 'edges':
        excluded = float((margin[fg] < ts.ORI_GUARD).mean())
        assert excluded <= ts.EDGE_EXCLUDED_CAP, 'edge masks: %.3f of the foreground inside the guard' % excluded
        assert all((margin[img == i] >= ts.ORI_GUARD).any() for i in ts.EDGE_IDS), 'an edge mask keeps no compared pixel'
      else:
        assert margin[fg].min() >= ts.ORI_GUARD, '%s image %d: orientation margin %.3g' % (name, b, margin[fg].min())
      key = '%s/%d/' % (name, b)
      arrays[key + 'class'], arrays[key + 'one_hot'] = cls, one_hot
      arrays[key + 'masks_packed'], arrays[key + 'masks_shape'] = ts.pack_masks(masks), np.array(masks.shape, np.int64)
      arrays[key + 'colours'] = colours
  write_npz(os.path.join(out, 'toolkit_orientation.npz'), arrays)
  for f in ('toolkit_instance.npz', 'toolkit_instance.json', 'toolkit_pixel.npz', 'toolkit_pixel.json', 'toolkit_orientation.npz'):
    print('%-26s %7d bytes' % (f, os.path.getsize(os.path.join(out, f))))


if __name__ == '__main__':
  main()
