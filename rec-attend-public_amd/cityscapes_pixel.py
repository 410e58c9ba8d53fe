#!/usr/bin/env python
"""Class IoU, category IoU and the instance-weighted iIoU of the Cityscapes pixel-level evaluation for label images any
method wrote: the interface of the reference's data_api/cityscapes_scripts/evaluation/evalPixelLevelSemanticLabeling.py
(cited as :line below), with the pixel work on the device.

  --pred DIR      the prediction tree: somewhere below it one 8-bit PNG '<city>_<seq>_<frame>*.png' per image whose values
                  are label ids (0 .. 33);
  --gt PATH       a folder searched for *_gtFine_labelIds.png (8-bit, utils/png.read_gray8), each with its
                  *_gtFine_instanceIds.png beside it (16-bit, read_gray16; :546), or an .npz with gt_instance_ids [N,H,W] and
                  names [N] (and optionally gt_label_ids uint8 [N,H,W]; without it a pixel's label is derived from its id:
                  id < 1000 ? id : id // 1000);
  --output FILE   where the result goes as JSON (default: <pred>/resultPixelLevelSemanticLabeling.json): the toolkit's keys
                  (:341-363) plus averageScorePredictedClasses, the mean class IoU over the eight thing labels.

A prediction belongs to a ground-truth image when its name starts with the image's '<city>_<seq>_<frame>' (:85-86); none or
several are errors (:88-97), and so is a prediction whose size differs from its ground truth (:553-557), named.  There is no
CPU path: without a GPU the script raises RecAttendError once the files of the first image have been read."""
import argparse
import fnmatch
import os

import numpy as np

from cityscapes_ap import image_stem
from ra_native import RecAttendError

MAX_BATCH_ELEMS = 1 << 28


def build_parser():
  p = argparse.ArgumentParser(description='Cityscapes pixel-level IoU / iIoU of a folder of label images')
  p.add_argument('--pred', required=True, help='folder holding one <city>_<seq>_<frame>*.png of label ids per image')
  p.add_argument('--gt', required=True, help='folder of *_gtFine_labelIds.png + *_gtFine_instanceIds.png, or an .npz with '
                                             'gt_instance_ids and names (+ gt_label_ids)')
  p.add_argument('--output', default=None, help='JSON file (default: <pred>/resultPixelLevelSemanticLabeling.json)')
  p.add_argument('--batch_size', type=int, default=4)
  return p


def list_ground_truth(path):
  """[(name, loader)] of --gt, in a fixed order; loader() -> (ids int32 [H,W], labels uint8 [H,W] or None)."""
  if os.path.isdir(path):
    from utils import png
    found = []
    for root, _, files in os.walk(path):
      found += [os.path.join(root, f) for f in fnmatch.filter(files, '*_gtFine_labelIds.png')]
    if not found:
      raise RecAttendError('no *_gtFine_labelIds.png below %s' % path)

    def load(f):
      inst = os.path.join(os.path.dirname(f), os.path.basename(f).replace('labelIds', 'instanceIds'))
      if not os.path.exists(inst):
        raise RecAttendError('Unable to load %s' % inst)
      labels, ids = png.read_gray8(f), png.read_gray16(inst).astype(np.int32)
      if labels.shape != ids.shape:
        raise RecAttendError('%s is %d x %d, %s is %d x %d' % ((f,) + labels.shape + (inst,) + ids.shape))
      return ids, labels
    return [(f, (lambda f=f: load(f))) for f in sorted(found)]
  data = np.load(path, allow_pickle=False)
  for k in ('gt_instance_ids', 'names'):
    if k not in data:
      raise RecAttendError('--gt %s lacks %s' % (path, k))
  ids = data['gt_instance_ids']
  labels = data['gt_label_ids'] if 'gt_label_ids' in data else None
  if ids.ndim != 3 or len(data['names']) != ids.shape[0]:
    raise RecAttendError('--gt %s: gt_instance_ids %s and %d names do not belong together' % (path, ids.shape, len(data['names'])))
  if labels is not None and (labels.shape != ids.shape or labels.dtype != np.uint8):
    raise RecAttendError('--gt %s: gt_label_ids is %s %s, expected uint8 %s' % (path, labels.dtype, labels.shape, ids.shape))
  return [(str(n), (lambda i=i: (np.asarray(ids[i], np.int32), None if labels is None else np.asarray(labels[i]))))
          for i, n in enumerate(data['names'])]


def find_prediction(walk, gt_name):
  """:85-99: the one PNG whose name starts with the image's stem."""
  pattern = image_stem(gt_name) + '*.png'
  hits = [os.path.join(root, f) for root, files in walk for f in fnmatch.filter(files, pattern)]
  if not hits:
    raise RecAttendError('Found no prediction for ground truth %s' % gt_name)
  if len(hits) > 1:
    raise RecAttendError('Found multiple predictions for ground truth %s: %s' % (gt_name, ', '.join(sorted(hits))))
  return hits[0]


def main(argv=None):
  from utils import png
  args = build_parser().parse_args(argv)
  gts = list_ground_truth(args.gt)
  walk = [(root, files) for root, _, files in os.walk(args.pred)]
  pairs = [(name, load, find_prediction(walk, name)) for name, load in gts]
  import analysis
  scorer = analysis.CityscapesPixelAnalyzer([name for name, _, _ in pairs])
  dev = None
  batch = []

  def flush():
    import torch
    res = {'pred': torch.from_numpy(np.stack([p for _, p, _, _ in batch])).to(dev),
           'gt_ids': torch.from_numpy(np.stack([g for _, _, g, _ in batch])).to(dev), 'indices': [i for i, _, _, _ in batch]}
    if batch[0][3] is not None:
      res['gt_labels'] = torch.from_numpy(np.stack([l for _, _, _, l in batch])).to(dev)
    scorer.stage(res)
    del batch[:]

  for index, (name, load, pred_file) in enumerate(pairs):
    ids, labels = load()
    ids = np.ascontiguousarray(ids, np.int32)
    pred = np.ascontiguousarray(png.read_gray8(pred_file))
    if pred.shape != ids.shape:  # :553-557
      raise RecAttendError('Image sizes of %s (%d x %d) and %s (%d x %d) are not equal' % ((pred_file,) + pred.shape + (name,) + ids.shape))
    if dev is None:  # the files of the first image are in order: from here on the device is needed
      from cityscapes_eval import _need_device
      torch = _need_device()
      dev = torch.device('cuda', torch.cuda.current_device())
    if batch and (batch[0][2].shape != ids.shape or len(batch) >= args.batch_size or (len(batch) + 1) * ids.size > MAX_BATCH_ELEMS):
      flush()
    batch.append((index, pred, ids, None if labels is None else np.ascontiguousarray(labels, np.uint8)))
  if batch:
    flush()
  out = args.output or os.path.join(args.pred, 'resultPixelLevelSemanticLabeling.json')
  result = scorer.finalize(out)
  print('%d images -> %s' % (len(pairs), out))
  return result


if __name__ == '__main__':
  main()
