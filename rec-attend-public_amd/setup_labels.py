#!/usr/bin/env python
"""The label stage of the reference's setup_cityscapes.py / setup_kitti.py / setup_cvppp.py (data_api/ins_seg_assembler.py:
85-155, sep_labels.py, orientation.py:31-85) with the pixel work on the device: from the instance-id image of every frame
to the ground truth the train and eval entry points read, as data_api/ins_seg_dataset.py:158-172,216-236,257-271 hands it to
them.

  --input PATH      an .npz with gt_instance_ids [N,Hf,Wf] (+ names [N], + optionally x [N,H,W,3] at network size, which is
                    passed through), or a folder searched for *.png: one-channel 8- or 16-bit label images (Cityscapes'
                    *_instanceIds.png), read with utils/png.py, all of one size;
  --dataset         cityscapes (an id is an instance iff id > 1000 and id // 1000 is one of the eight instance labels; nine
                    semantic channels) | kitti | cvppp (every id != 0 is an instance; one semantic channel);
  --height, --width, --timespan   the network size and the number of instance slots (default: the dataset's,
                    cmd_args_parser.INP_DIM);
  --target          full_model -> y_gt [N,T,H,W], s_gt [N,T] (+ x): an --input of full_model_train.py / box_model_train.py;
                    fg_model   -> y_gt [N,H,W,nsc] (the semantic map c_gt), d_gt [N,H,W,8], fg_gt_full [N,Hf,Wf] uint8, names
                                  (+ x): an --input of fg_model_eval.py;
                    all        -> y_gt_ins, s_gt, c_gt, d_gt, d_cls, fg_gt_full, inst_id, area, sem_cls, num_obj, names (+ x);
  --output FILE     the .npz that is written.

The instances of an image are sorted by their area at network size, descending; equal areas put the larger id first
(DESIGN.md).  Limits, stated: colour label images (the three-channel files of CVPPP and KITTI: pack the colour into an id in
[1, 65535] yourself), the INTER_CUBIC resize of the colour image to network size (bring x at network size, or none) and HDF5
output are not built.  An image with more than ra_ops.MAX_GT distinct ids or an id above 65535 is an error that names it.
There is no CPU path: without a GPU the script raises RecAttendError once the input has been read."""
import argparse
import fnmatch
import os

import numpy as np

import cmd_args_parser as cap
from ra_native import RecAttendError

MAX_BATCH_ELEMS = 1 << 28  # floats of one batch's y_gt
TARGETS = {
    'full_model': {'y_gt': 'y_gt', 's_gt': 's_gt'},
    'fg_model': {'y_gt': 'c_gt', 'd_gt': 'd_gt', 'fg_gt_full': 'fg_gt_full'},
    'all': {'y_gt_ins': 'y_gt', 's_gt': 's_gt', 'c_gt': 'c_gt', 'd_gt': 'd_gt', 'd_cls': 'd_cls', 'fg_gt_full': 'fg_gt_full',
            'inst_id': 'inst_id', 'area': 'area', 'sem_cls': 'sem_cls', 'num_obj': 'num_obj'},
}  # archive key -> ra_ops.assemble_labels output


def build_parser():
  p = argparse.ArgumentParser(description='Assemble y_gt, s_gt, d_gt, c_gt from instance-id images')
  p.add_argument('--input', required=True, help='.npz with gt_instance_ids [N,Hf,Wf] (+ names, x), or a folder of label PNG files')
  p.add_argument('--dataset', required=True, choices=('cityscapes', 'kitti', 'cvppp'))
  p.add_argument('--height', type=int, default=None)
  p.add_argument('--width', type=int, default=None)
  p.add_argument('--timespan', type=int, default=None)
  p.add_argument('--target', default='full_model', choices=sorted(TARGETS))
  p.add_argument('--output', required=True, help='the .npz to write')
  p.add_argument('--batch_size', type=int, default=8)
  return p


def read_label_png(path):
  """A one-channel, non-interlaced 8- or 16-bit PNG -> int32 [Hf,Wf]."""
  from utils import png
  with open(path, 'rb') as f:
    data = f.read()
  if len(data) < 26 or data[:8] != png.SIGNATURE:
    raise RecAttendError('%s is not a PNG file' % path)
  depth, colour = data[24], data[25]
  if colour != 0 or depth not in (8, 16):
    raise RecAttendError('%s: colour type %d, bit depth %d — only one-channel 8- or 16-bit label images are read (pack a colour '
                         'label image into ids in [1, 65535] first)' % (path, colour, depth))
  try:
    return (png.decode_gray16(data) if depth == 16 else png.decode_gray8(data)).astype(np.int32)
  except ValueError as e:
    raise RecAttendError('%s: %s' % (path, e))


def load_input(path):
  """-> (gt_instance_ids integer [N,Hf,Wf], names [N], x or None)"""
  if os.path.isdir(path):
    found = []
    for root, _, files in os.walk(path):
      found += [os.path.join(root, f) for f in fnmatch.filter(files, '*.png')]
    if not found:
      raise RecAttendError('no *.png below %s' % path)
    found.sort()
    imgs = [read_label_png(f) for f in found]
    if len({im.shape for im in imgs}) != 1:
      raise RecAttendError('%s: the label images have different sizes (%s); one full size per run' % (
          path, ', '.join(sorted({'%dx%d' % im.shape for im in imgs}))))
    return np.stack(imgs), [os.path.basename(f) for f in found], None
  data = np.load(path, allow_pickle=False)
  if 'gt_instance_ids' not in data:
    raise RecAttendError('--input %s lacks gt_instance_ids' % path)
  ids = data['gt_instance_ids']
  if ids.ndim != 3 or not np.issubdtype(ids.dtype, np.integer):
    raise RecAttendError('--input %s: gt_instance_ids is %s %s, expected integers [N,Hf,Wf]' % (path, ids.dtype, tuple(ids.shape)))
  names = [str(n) for n in data['names']] if 'names' in data else ['image_%06d' % i for i in range(ids.shape[0])]
  if len(names) != ids.shape[0]:
    raise RecAttendError('--input %s: %d names for %d images' % (path, len(names), ids.shape[0]))
  return ids, names, (data['x'] if 'x' in data else None)


def assemble_archive(ids, names, x, dataset, H, W, T, target, batch_size=8):
  """{archive key: array} of --target for ids [N,Hf,Wf]."""
  import torch
  import ra_ops as ops
  N, Hf, Wf = ids.shape
  if not (1 <= T <= ops.LABELS_MAX_T and 1 <= H <= Hf and 1 <= W <= Wf):
    raise RecAttendError('--height %d --width %d --timespan %d for label images of %d x %d (1 <= timespan <= %d, the network '
                         'size no larger than the labels)' % (H, W, T, Hf, Wf, ops.LABELS_MAX_T))
  if x is not None and tuple(x.shape[:3]) != (N, H, W):
    raise RecAttendError('--input: x is %s, expected [%d,%d,%d,3] at network size (the resize of the colour image is not '
                         'built)' % (tuple(x.shape), N, H, W))
  if not torch.cuda.is_available():
    raise RecAttendError('setup_labels runs on the GPU; no device is available and there is no CPU fallback')
  keys = TARGETS[target]
  bs = max(1, min(int(batch_size), MAX_BATCH_ELEMS // max(1, T * H * W), MAX_BATCH_ELEMS // max(1, Hf * Wf)))
  parts = {k: [] for k in keys}
  for b0 in range(0, N, bs):
    got = ops.assemble_labels(np.asarray(ids[b0:b0 + bs]), H, W, T, dataset, want=tuple(sorted(set(keys.values()))),
                              names=names[b0:b0 + bs])
    for k, src in keys.items():
      parts[k].append(got[src].cpu().numpy())
  out = {k: np.concatenate(v) for k, v in parts.items()}
  if target != 'full_model':
    out['names'] = np.asarray(names)
  if x is not None:
    out['x'] = np.asarray(x, np.float32)
  return out


def main(argv=None):
  args = build_parser().parse_args(argv)
  h, w, t = cap.INP_DIM[args.dataset]
  H, W, T = args.height or h, args.width or w, args.timespan or t
  ids, names, x = load_input(args.input)
  out = assemble_archive(ids, names, x, args.dataset, H, W, T, args.target, args.batch_size)
  folder = os.path.dirname(os.path.abspath(args.output))
  os.makedirs(folder, exist_ok=True)
  np.savez(args.output, **out)
  print('%d images, %d x %d -> %d x %d, timespan %d -> %s (%s)' % (ids.shape[0], ids.shape[1], ids.shape[2], H, W, T, args.output,
                                                                 ', '.join(sorted(out))))
  return out


if __name__ == '__main__':
  main()
