#!/usr/bin/env python
"""AP and AP50% of the Cityscapes instance-level evaluation for result files any method wrote: the interface of the
reference's data_api/cityscapes_scripts/evaluation/evalInstanceLevelSemanticLabeling.py (run_cityscapes_eval.sh:51; cited
as :line below), with the pixel work on the device.

  --results DIR   the prediction tree: somewhere below it one '<city>_<seq>_<frame>*.txt' per image, every line
                  '<mask file relative to the text file> <label id> <confidence>' (:165-189), every mask an 8-bit PNG whose
                  non-zero pixels are the instance (what analysis.RenderCityScapesOutputAnalyzer writes);
  --gt PATH       an .npz with gt_instance_ids [N,H,W] and names [N], or a folder searched for *_gtFine_instanceIds.png
                  (16-bit PNG files, read with utils/png.read_gray16);
  --output FILE   where the result goes as JSON (default: <results>/resultInstanceLevelSemanticLabeling.json).

A prediction file belongs to a ground-truth image when its name starts with the image's '<city>_<seq>_<frame>' (:90-95); none
or several are errors (:96-102), and so are a line that does not have three fields, an absolute mask path, a mask outside
--results (:172-182) and a mask whose size differs from the ground truth.  An image may list any number of predictions (the
scorer runs the overlap kernel once per 32 of them).  Distance-conditioned figures (AP50m, AP100m) are not computed.  There is no CPU path: without a
GPU the script raises RecAttendError once the files have been read."""
import argparse
import fnmatch
import os

import numpy as np

from ra_native import RecAttendError

MAX_BATCH_ELEMS = 1 << 28


def build_parser():
  p = argparse.ArgumentParser(description='Cityscapes instance-level AP of a folder of result files')
  p.add_argument('--results', required=True, help='folder holding <run>/<name>.txt and the mask PNG files')
  p.add_argument('--gt', required=True, help='.npz with gt_instance_ids and names, or a folder of *_gtFine_instanceIds.png')
  p.add_argument('--output', default=None, help='JSON file (default: <results>/resultInstanceLevelSemanticLabeling.json)')
  p.add_argument('--batch_size', type=int, default=4)
  return p


def image_stem(name):
  """'<city>_<seq>_<frame>' of a ground-truth or image file name (csHelpers.getCsFileInfo: the first three '_' fields)."""
  base = os.path.basename(str(name))
  base = base[:-4] if base.endswith('.png') else base
  parts = base.split('_')
  if len(parts) < 3:
    raise RecAttendError('%s is not a Cityscapes file name (<city>_<seq>_<frame>...)' % name)
  return '_'.join(parts[:3])


def list_ground_truth(path):
  """[(name, loader)] of --gt, in a fixed order; loader() -> int32 [H,W]."""
  if os.path.isdir(path):
    from utils import png
    found = []
    for root, _, files in os.walk(path):
      found += [os.path.join(root, f) for f in fnmatch.filter(files, '*_gtFine_instanceIds.png')]
    if not found:
      raise RecAttendError('no *_gtFine_instanceIds.png below %s' % path)
    return [(f, (lambda f=f: png.read_gray16(f).astype(np.int32))) for f in sorted(found)]
  data = np.load(path, allow_pickle=False)
  for k in ('gt_instance_ids', 'names'):
    if k not in data:
      raise RecAttendError('--gt %s lacks %s' % (path, k))
  ids = data['gt_instance_ids']
  if ids.ndim != 3 or len(data['names']) != ids.shape[0]:
    raise RecAttendError('--gt %s: gt_instance_ids %s and %d names do not belong together' % (path, ids.shape, len(data['names'])))
  return [(str(n), (lambda i=i: np.asarray(ids[i], np.int32))) for i, n in enumerate(data['names'])]


def find_prediction(walk, gt_name):
  """:90-102: the one text file whose name starts with the image's stem."""
  pattern = image_stem(gt_name) + '*.txt'
  hits = [os.path.join(root, f) for root, files in walk for f in fnmatch.filter(files, pattern)]
  if not hits:
    raise RecAttendError('Found no prediction for ground truth %s' % gt_name)
  if len(hits) > 1:
    raise RecAttendError('Found multiple predictions for ground truth %s: %s' % (gt_name, ', '.join(sorted(hits))))
  return hits[0]


def read_prediction_file(text_file, root):
  """:165-189 -> [(mask file, label id, confidence)]."""
  root = os.path.abspath(root)
  out = []
  with open(text_file) as f:
    for line in f:
      parts = line.split(' ')
      if len(parts) != 3:
        raise RecAttendError('%s: a line needs three fields, "<mask file> <label id> <confidence>", got %r' % (text_file, line))
      if os.path.isabs(parts[0]):
        raise RecAttendError('%s: the mask file %s must be given relative to the text file' % (text_file, parts[0]))
      mask = os.path.abspath(os.path.join(os.path.dirname(text_file), parts[0]))
      if os.path.commonpath([mask, root]) != root:
        raise RecAttendError('%s: the mask file %s lies outside %s' % (text_file, mask, root))
      out.append((mask, int(float(parts[1])), float(parts[2])))
  return out


def load_image(gt_name, gt, text_file, root):
  """-> (y float32 [T,H,W] of 0 / 1, label_id [T], conf float64 [T]) of one image's predictions."""
  from utils import png
  lines = read_prediction_file(text_file, root)
  y = np.zeros((len(lines),) + gt.shape, np.float32)
  for t, (mask_file, _, _) in enumerate(lines):
    mask = png.read_gray8(mask_file)
    if mask.shape != gt.shape:
      raise RecAttendError('%s is %d x %d, the ground truth %s is %d x %d' % ((mask_file,) + mask.shape + (gt_name,) + gt.shape))
    y[t] = mask != 0
  return y, np.array([l for _, l, _ in lines], np.int32), np.array([c for _, _, c in lines], np.float64)


def main(argv=None):
  args = build_parser().parse_args(argv)
  gts = list_ground_truth(args.gt)
  walk = [(root, files) for root, _, files in os.walk(args.results)]
  pairs = [(name, load, find_prediction(walk, name)) for name, load in gts]
  import analysis
  scorer = analysis.CityscapesAPAnalyzer([name for name, _, _ in pairs])
  dev = None
  batch = []

  def flush():
    import torch
    T = max(1, max(item[1].shape[0] for item in batch))
    H, W = batch[0][2].shape
    y = np.zeros((len(batch), T, H, W), np.float32)
    lab = np.full((len(batch), T), -1, np.int32)
    conf = np.zeros((len(batch), T), np.float64)
    for i, (_, yi, _, li, ci) in enumerate(batch):
      y[i, :yi.shape[0]], lab[i, :li.size], conf[i, :ci.size] = yi, li, ci
    scorer.stage({'y_out': torch.from_numpy(y).to(dev), 'gt_ids': torch.from_numpy(np.stack([g for _, _, g, _, _ in batch])).to(dev),
                  'label_id': lab, 'conf': conf, 'indices': [i for i, _, _, _, _ in batch]})
    del batch[:]

  for index, (name, load, text_file) in enumerate(pairs):
    gt = np.ascontiguousarray(load(), np.int32)
    y, lab, conf = load_image(name, gt, text_file, args.results)
    if dev is None:  # the files of the first image are in order: from here on the device is needed
      from cityscapes_eval import _need_device
      torch = _need_device()
      dev = torch.device('cuda', torch.cuda.current_device())
    if batch and (batch[0][2].shape != gt.shape or len(batch) >= args.batch_size or
                  (len(batch) + 1) * max([y.shape[0]] + [item[1].shape[0] for item in batch]) * gt.size > MAX_BATCH_ELEMS):
      flush()
    batch.append((index, y, gt, lab, conf))
  if batch:
    flush()
  out = args.output or os.path.join(args.results, 'resultInstanceLevelSemanticLabeling.json')
  result = scorer.finalize(out)
  print('%d images -> %s' % (len(pairs), out))
  return result


if __name__ == '__main__':
  main()
