#!/usr/bin/env python
"""The label stage of the reference's setup_cityscapes.py / setup_kitti.py / setup_cvppp.py (data_api/ins_seg_assembler.py:
85-155, sep_labels.py, orientation.py:31-85) with the pixel work on the device: from the instance-id image of every frame
to the ground truth the train and eval entry points read, as data_api/ins_seg_dataset.py:158-172,216-236,257-271 hands it to
them.

  --input PATH      an .npz with gt_instance_ids [N,Hf,Wf] (+ names [N], + optionally x [N,H,W,3] at network size, which is
                    passed through, or x_full uint8 [N,Hf,Wf,3] and no x, which is resized to x as --images does), or a
                    folder searched for *.png: one-channel 8- or 16-bit label images (Cityscapes' *_instanceIds.png), read
                    with utils/png.py, all of one size;
  --images DIR      (opt-in) the colour image of every label file, read with utils/png.read_colour8 (uint8, cv2's BGR order)
                    and resized to network size on the device in batches (ra_ops.resize_cubic, the INTER_CUBIC of
                    ins_seg_assembler.py:116): the archive then holds x float32 [N,H,W,3] (BGR, / 255) and orig_size int32
                    [N,2].  The label folder is then filtered by the dataset's label pattern, and the image is
                      cityscapes  <key>_leftImg8bit.png anywhere below DIR for <key>_gtFine_instanceIds.png,
                      kitti       the label file's basename below DIR,
                      cvppp       plantNNN_rgb.png for plantNNN_label.png (DIR may be --input itself);
                    where DIR holds the name more than once, the one in the label's own sub-folder.  A label without an
                    image, or an image whose size is not its label's, is an error that names the file;
  --colour_labels   (opt-in) label files may be colour PNG files (CVPPP's and KITTI's, cvppp.py:58, kitti.py:57): per image
                    code = B << 16 | G << 8 | R (sep_labels.py:15 on cv2's BGR array), the distinct non-zero codes in
                    ascending order become the ids 1, 2, ... and 0 stays 0, on the host (np.unique).  Grey files pass
                    through unchanged;
  --dataset         cityscapes (an id is an instance iff id > 1000 and id // 1000 is one of the eight instance labels; nine
                    semantic channels) | kitti | cvppp (every id != 0 is an instance; one semantic channel);
  --height, --width, --timespan   the network size and the number of instance slots (default: the dataset's,
                    cmd_args_parser.INP_DIM);
  --target          full_model -> y_gt [N,T,H,W], s_gt [N,T] (+ x): an --input of full_model_train.py / box_model_train.py;
                    fg_model   -> y_gt [N,H,W,nsc] (the semantic map c_gt), d_gt [N,H,W,8], fg_gt_full [N,Hf,Wf] uint8, names
                                  (+ x): an --input of fg_model_eval.py;
                    all        -> y_gt_ins, s_gt, c_gt, d_gt, d_cls, fg_gt_full, inst_id, area, sem_cls, num_obj, names (+ x);
  --mixed_sizes     (opt-in, NOT in the reference, whose setup scripts resize image by image on the host) the label files of
                    the folder may differ in size, as KITTI's do.  The archive then holds, next to the network-size labels of
                    --target, which stay dense, the ids in the flat layout of include/recattend.h (ra_image_geo):
                    gt_instance_ids_flat int32 [P], pixel_offset int64 [N + 1] (image i starts at element pixel_offset[i], a
                    multiple of 4, rows packed with pitch w; pixel_offset[N] = P) and orig_size int32 [N,2], which now varies
                    per image; --target fg_model / all hold fg_gt_full_flat uint8 [P] at the same offsets in place of
                    fg_gt_full.  Every batch goes through ONE launch chain (ra_ops.assemble_labels_ragged).  With --images the
                    colour images are grouped by size on the host and each group is resized through the same
                    ra_resize_cubic_u8 launches as before: the cubic tables are per (source size, network size) anyway and this
                    stage is offline, so there is no ragged resize kernel.  Such an archive is an --input of full_model_eval.py,
                    fg_model_eval.py, full_model_train.py and box_model_train.py;
  --output FILE     the .npz that is written.

The instances of an image are sorted by their area at network size, descending; equal areas put the larger id first
(DESIGN.md).  Limits, stated: without the two flags a colour label image is refused (pack the colour into an id in [1, 65535]
yourself) and x comes at network size or not at all; colour files are 8-bit and not interlaced, x is in BGR order; all
images and labels of a run have ONE full size unless --mixed_sizes is given (without it mixed sizes are refused: "one full size
per run"); HDF5 output is not built.
The resize equals the recipe include/recattend.h restates from cv2's source, not a cv2 that was run.  An image with more than
ra_ops.MAX_GT distinct ids (under --colour_labels: more than MAX_GT - 1 colours) or an id above 65535 is an error that names it.
There is no CPU path: without a GPU the script raises RecAttendError once the input has been read."""
import argparse
import fnmatch
import os
import re

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
LABEL_PATTERNS = {'cityscapes': '*_gtFine_instanceIds.png', 'kitti': '*.png', 'cvppp': 'plant*_label.png'}  # under --images


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
  p.add_argument('--images', default=None, help='folder of the colour images: resized to x at network size on the device')
  p.add_argument('--colour_labels', action='store_true', help='label files may be colour PNG files: colours become ids')
  p.add_argument('--mixed_sizes', action='store_true', help='label files may differ in size (KITTI): the ids are kept in one flat '
                 'buffer with per-image offsets and sizes.  Not a flag of the reference, which resizes image by image on the host')
  return p


def colour_ids(bgr, path):
  """sep_labels.py:12-26 on cv2's BGR array: uint8 [Hf,Wf,3] -> int32 ids, 0 for the code 0 and 1, 2, ... for the other
  distinct codes B << 16 | G << 8 | R in ascending order."""
  import ra_ops as ops
  code = (bgr[:, :, 0].astype(np.int32) << 16) | (bgr[:, :, 1].astype(np.int32) << 8) | bgr[:, :, 2]
  codes, inverse = np.unique(code, return_inverse=True)
  n = len(codes) - (1 if codes[0] == 0 else 0)
  if n > ops.MAX_GT - 1:
    raise RecAttendError('%s: %d distinct colours, at most %d are instances of one image' % (path, n, ops.MAX_GT - 1))
  first = 0 if codes[0] == 0 else 1  # the id of the smallest code
  return (inverse.reshape(code.shape) + first).astype(np.int32)


def read_label_png(path, colour_labels=False):
  """A one-channel, non-interlaced 8- or 16-bit PNG -> int32 [Hf,Wf]; with colour_labels also a colour PNG (colour_ids)."""
  from utils import png
  with open(path, 'rb') as f:
    data = f.read()
  if len(data) < 26 or data[:8] != png.SIGNATURE:
    raise RecAttendError('%s is not a PNG file' % path)
  depth, colour = data[24], data[25]
  if colour_labels and not (colour == 0 and depth in (8, 16)):
    try:
      return colour_ids(png.decode_colour8(data), path)
    except ValueError as e:
      raise RecAttendError('%s: %s' % (path, e))
  if colour != 0 or depth not in (8, 16):
    raise RecAttendError('%s: colour type %d, bit depth %d — only one-channel 8- or 16-bit label images are read (pack a colour '
                         'label image into ids in [1, 65535] first)' % (path, colour, depth))
  try:
    return (png.decode_gray16(data) if depth == 16 else png.decode_gray8(data)).astype(np.int32)
  except ValueError as e:
    raise RecAttendError('%s: %s' % (path, e))


def find_files(path, pattern='*.png'):
  """The files below `path` whose name matches `pattern`, sorted."""
  found = []
  for root, _, files in os.walk(path):
    found += [os.path.join(root, f) for f in fnmatch.filter(files, pattern)]
  return sorted(found)


def image_name(dataset, label_name):
  """The colour image's file name for a label file's (ins_seg_assembler.py's datasets: cityscapes.py, kitti.py, cvppp.py:41)."""
  if dataset == 'cityscapes':
    return label_name[:-len('_gtFine_instanceIds.png')] + '_leftImg8bit.png'
  if dataset == 'cvppp':
    return re.sub(r'_label\.png$', '_rgb.png', label_name)
  return label_name


def pair_images(label_paths, label_root, image_root, dataset):
  """The colour image of every label file below image_root: by name; of several of one name, the one whose sub-folder of
  image_root is the label's sub-folder of label_root."""
  by_name = {}
  for f in find_files(image_root):
    by_name.setdefault(os.path.basename(f), []).append(f)
  out = []
  for lab in label_paths:
    name = image_name(dataset, os.path.basename(lab))
    cands = [c for c in by_name.get(name, []) if os.path.abspath(c) != os.path.abspath(lab)]
    if len(cands) > 1:
      sub = os.path.relpath(os.path.dirname(lab), label_root)
      cands = [c for c in cands if os.path.relpath(os.path.dirname(c), image_root) == sub] or cands
    if len(cands) != 1:
      raise RecAttendError('%s: %s %s below %s' % (lab, 'more than one image' if cands else 'no image', name, image_root))
    out.append(cands[0])
  return out


FLAT_ALIGN = 4  # elements: ra_ops.RAGGED_ALIGN, every image of a flat archive starts at a multiple


def flatten_images(imgs):
  """A list of integer [h,w] arrays -> {'gt_instance_ids_flat' int32 [P], 'pixel_offset' int64 [N + 1], 'orig_size' int32 [N,2]}:
  the flat layout of --mixed_sizes (host code; ra_ops.pack_ragged's layout)."""
  offset = np.zeros(len(imgs) + 1, np.int64)
  for i, im in enumerate(imgs):
    offset[i + 1] = -(-(int(offset[i]) + im.size) // FLAT_ALIGN) * FLAT_ALIGN
  flat = np.zeros(int(offset[-1]), np.int32)
  for i, im in enumerate(imgs):
    flat[offset[i]:offset[i] + im.size] = im.reshape(-1)
  return {'gt_instance_ids_flat': flat, 'pixel_offset': offset, 'orig_size': np.array([im.shape for im in imgs], np.int32).reshape(-1, 2)}


def check_flat(where, flat, offset, size, n_names=None):
  """The flat layout's own consistency (host code): raises RecAttendError naming the image."""
  if flat.ndim != 1 or offset.ndim != 1 or size.ndim != 2 or size.shape[1] != 2 or len(offset) != len(size) + 1 or len(size) < 1:
    raise RecAttendError('%s: flat %s, pixel_offset %s, orig_size %s; expected [P], [N + 1], [N,2]' % (
        where, tuple(flat.shape), tuple(offset.shape), tuple(size.shape)))
  if n_names is not None and n_names != len(size):
    raise RecAttendError('%s: %d names for %d images' % (where, n_names, len(size)))
  for i in range(len(size)):
    h, w = int(size[i, 0]), int(size[i, 1])
    if h < 1 or w < 1 or int(offset[i]) < 0 or int(offset[i]) + h * w > int(offset[i + 1]) or int(offset[i + 1]) > flat.shape[0]:
      raise RecAttendError('%s: image %d is %d x %d at element %d, the next one starts at %d of %d' % (
          where, i, h, w, int(offset[i]), int(offset[i + 1]), flat.shape[0]))


def flat_geometry(offset, size, b0, b1):
  """The geometry [b1 - b0, 3] (offset, h, w) of the images b0 .. b1 - 1 within flat[offset[b0]:offset[b1]]."""
  return np.concatenate([(np.asarray(offset[b0:b1], np.int64) - int(offset[b0]))[:, None], np.asarray(size[b0:b1], np.int64)], axis=1)


def load_input(path, pattern='*.png', colour_labels=False, want_paths=False, mixed_sizes=False):
  """-> (gt_instance_ids integer [N,Hf,Wf], names [N], x or None); want_paths: the files' paths in place of the names.
  mixed_sizes: the label images may differ in size, and the first item is the flat structure of flatten_images instead (from
  a folder; from an .npz that holds gt_instance_ids_flat, pixel_offset and orig_size; or from gt_instance_ids [N,Hf,Wf])."""
  if os.path.isdir(path):
    found = find_files(path, pattern)
    if not found:
      raise RecAttendError('no %s below %s' % (pattern, path))
    imgs = [read_label_png(f, colour_labels) for f in found]
    if mixed_sizes:
      return flatten_images(imgs), (found if want_paths else [os.path.basename(f) for f in found]), None
    if len({im.shape for im in imgs}) != 1:
      raise RecAttendError('%s: the label images have different sizes (%s); one full size per run' % (
          path, ', '.join(sorted({'%dx%d' % im.shape for im in imgs}))))
    return np.stack(imgs), (found if want_paths else [os.path.basename(f) for f in found]), None
  data = np.load(path, allow_pickle=False)
  if mixed_sizes and 'gt_instance_ids_flat' in data:
    missing = [k for k in ('pixel_offset', 'orig_size') if k not in data]
    if missing:
      raise RecAttendError('--input %s holds gt_instance_ids_flat and lacks %s' % (path, ', '.join(missing)))
    flat = {k: data[k] for k in ('gt_instance_ids_flat', 'pixel_offset', 'orig_size')}
    names = [str(n) for n in data['names']] if 'names' in data else ['image_%06d' % i for i in range(len(flat['orig_size']))]
    check_flat('--input %s' % path, flat['gt_instance_ids_flat'], flat['pixel_offset'], flat['orig_size'], len(names))
    return flat, names, (data['x'] if 'x' in data else None)
  if 'gt_instance_ids' not in data:
    raise RecAttendError('--input %s lacks gt_instance_ids' % path)
  ids = data['gt_instance_ids']
  if ids.ndim != 3 or not np.issubdtype(ids.dtype, np.integer):
    raise RecAttendError('--input %s: gt_instance_ids is %s %s, expected integers [N,Hf,Wf]' % (path, ids.dtype, tuple(ids.shape)))
  names = [str(n) for n in data['names']] if 'names' in data else ['image_%06d' % i for i in range(ids.shape[0])]
  if len(names) != ids.shape[0]:
    raise RecAttendError('--input %s: %d names for %d images' % (path, len(names), ids.shape[0]))
  if mixed_sizes:
    return flatten_images(list(ids)), names, (data['x'] if 'x' in data else None)
  return ids, names, (data['x'] if 'x' in data else None)


def assemble_archive_mixed(flat, names, x, dataset, H, W, T, target, batch_size=8):
  """{archive key: array} of --target for the flat structure of load_input(..., mixed_sizes=True): the network-size labels
  dense as assemble_archive has them, fg_gt_full as fg_gt_full_flat, and the flat ids with their offsets and sizes.  One
  ra_ops.assemble_labels_ragged call per batch."""
  import torch
  import ra_ops as ops
  ids, offset, size = flat['gt_instance_ids_flat'], flat['pixel_offset'], flat['orig_size']
  N = len(size)
  check_flat('--input', ids, offset, size, len(names))
  small = [i for i in range(N) if H > size[i, 0] or W > size[i, 1]]
  if not 1 <= T <= ops.LABELS_MAX_T or H < 1 or W < 1 or small:
    raise RecAttendError('--height %d --width %d --timespan %d%s (1 <= timespan <= %d, the network size no larger than any label '
                         'image)' % (H, W, T, ' for the label image %s of %d x %d' % (names[small[0]], size[small[0], 0],
                                                                                     size[small[0], 1]) if small else '',
                                     ops.LABELS_MAX_T))
  if x is not None and tuple(x.shape[:3]) != (N, H, W):
    raise RecAttendError('--input: x is %s, expected [%d,%d,%d,3] at network size' % (tuple(x.shape), N, H, W))
  if not torch.cuda.is_available():
    raise RecAttendError('setup_labels runs on the GPU; no device is available and there is no CPU fallback')
  keys = TARGETS[target]
  bs = max(1, min(int(batch_size), MAX_BATCH_ELEMS // max(1, T * H * W)))
  parts = {k: [] for k in keys}
  for b0 in range(0, N, bs):
    b1 = min(N, b0 + bs)
    gt = torch.from_numpy(np.ascontiguousarray(ids[int(offset[b0]):int(offset[b1])], np.int32)).cuda()
    got = ops.assemble_labels_ragged(gt, flat_geometry(offset, size, b0, b1), H, W, T, dataset,
                                     want=tuple(sorted(set(keys.values()))), names=names[b0:b1])
    for k, src in keys.items():
      parts[k].append(got[src].cpu().numpy())
  out = {('fg_gt_full_flat' if k == 'fg_gt_full' else k): np.concatenate(v) for k, v in parts.items()}
  out.update(gt_instance_ids_flat=np.asarray(ids, np.int32), pixel_offset=np.asarray(offset, np.int64), orig_size=np.asarray(size, np.int32))
  if target != 'full_model':
    out['names'] = np.asarray(names)
  if x is not None:
    out['x'] = np.asarray(x, np.float32)
  return out


def resize_images_mixed(read, size, H, W, batch_size=8):
  """x float32 [N,H,W,3] of N full-size images read(i) of the sizes size [N,2]: grouped by size on the host, every group through
  resize_images (the cubic tables are per (source size, network size); this stage is offline)."""
  x = np.zeros((len(size), H, W, 3), np.float32)
  groups = {}
  for i, hw in enumerate(np.asarray(size).tolist()):
    groups.setdefault(tuple(hw), []).append(i)
  for full, members in sorted(groups.items()):
    x[members] = resize_images(lambda j: read(members[j]), len(members), full, H, W, batch_size)
  return x


def assemble_archive(ids, names, x, dataset, H, W, T, target, batch_size=8):
  """{archive key: array} of --target for ids [N,Hf,Wf]."""
  import torch
  import ra_ops as ops
  N, Hf, Wf = ids.shape
  if not (1 <= T <= ops.LABELS_MAX_T and 1 <= H <= Hf and 1 <= W <= Wf):
    raise RecAttendError('--height %d --width %d --timespan %d for label images of %d x %d (1 <= timespan <= %d, the network '
                         'size no larger than the labels)' % (H, W, T, Hf, Wf, ops.LABELS_MAX_T))
  if x is not None and tuple(x.shape[:3]) != (N, H, W):
    raise RecAttendError('--input: x is %s, expected [%d,%d,%d,3] at network size (full-size images are resized under '
                         '--images, or from x_full in place of x)' % (tuple(x.shape), N, H, W))
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


def resize_images(read, N, full, H, W, batch_size=8):
  """x float32 [N,H,W,3] of the N full-size images read(i) -> uint8 [Hf,Wf,3] (every one of size `full`, or read raises):
  ra_ops.resize_cubic on the device, batch_size images at a time, so that the full-size images never exist together."""
  import torch
  import ra_ops as ops
  if not torch.cuda.is_available():
    raise RecAttendError('setup_labels runs on the GPU; no device is available and there is no CPU fallback')
  bs = max(1, min(int(batch_size), MAX_BATCH_ELEMS // max(1, full[0] * full[1] * 3), MAX_BATCH_ELEMS // max(1, H * W * 3)))
  parts = []
  for b0 in range(0, N, bs):
    batch = np.stack([read(i) for i in range(b0, min(N, b0 + bs))])
    parts.append(ops.resize_cubic(batch, H, W, want=('x',))['x'].cpu().numpy())
  return np.concatenate(parts)


def read_image_of(label_path, image_path, full):
  """The colour image of a label file, uint8 [Hf,Wf,3] BGR, checked against the labels' size."""
  from utils import png
  try:
    img = png.read_colour8(image_path)
  except ValueError as e:
    raise RecAttendError('%s: %s' % (image_path, e))
  if tuple(img.shape[:2]) != tuple(full):
    raise RecAttendError('%s is %d x %d, its label image %s %d x %d' % (image_path, img.shape[0], img.shape[1], label_path,
                                                                       full[0], full[1]))
  return img


def main(argv=None):
  args = build_parser().parse_args(argv)
  h, w, t = cap.INP_DIM[args.dataset]
  H, W, T = args.height or h, args.width or w, args.timespan or t
  orig_size = None
  if args.mixed_sizes:
    pattern = LABEL_PATTERNS[args.dataset] if args.images else '*.png'
    flat, paths, x = load_input(args.input, pattern, args.colour_labels, want_paths=True, mixed_sizes=True)
    names = [os.path.basename(f) for f in paths]
    if args.images:
      if not os.path.isdir(args.input) or not os.path.isdir(args.images):
        raise RecAttendError('--images %s needs folders for --input and --images' % args.images)
      images, size = pair_images(paths, args.input, args.images, args.dataset), flat['orig_size']
      x = resize_images_mixed(lambda i: read_image_of(paths[i], images[i], tuple(size[i])), size, H, W, args.batch_size)
    out = assemble_archive_mixed(flat, names, x, args.dataset, H, W, T, args.target, args.batch_size)
    os.makedirs(os.path.dirname(os.path.abspath(args.output)), exist_ok=True)
    np.savez(args.output, **out)
    sizes = sorted({'%dx%d' % tuple(hw) for hw in out['orig_size'].tolist()})
    print('%d images of %d sizes (%s) -> %d x %d, timespan %d -> %s (%s)' % (len(names), len(sizes), ', '.join(sizes[:6]), H, W, T,
                                                                           args.output, ', '.join(sorted(out))))
    return out
  if args.images:
    if not os.path.isdir(args.input) or not os.path.isdir(args.images):
      raise RecAttendError('--images %s needs folders for --input and --images' % args.images)
    ids, paths, _ = load_input(args.input, LABEL_PATTERNS[args.dataset], args.colour_labels, want_paths=True)
    images = pair_images(paths, args.input, args.images, args.dataset)
    names, full = [os.path.basename(f) for f in paths], ids.shape[1:]
    x = resize_images(lambda i: read_image_of(paths[i], images[i], full), len(paths), full, H, W, args.batch_size)
    orig_size = np.tile(np.asarray(full, np.int32), (len(paths), 1))
  else:
    ids, names, x = load_input(args.input, colour_labels=args.colour_labels)
    x_full = None
    if x is None and not os.path.isdir(args.input):
      data = np.load(args.input, allow_pickle=False)
      x_full = data['x_full'] if 'x_full' in data else None
    if x_full is not None:
      if x_full.dtype != np.uint8 or x_full.ndim != 4 or x_full.shape[3] != 3 or tuple(x_full.shape[:3]) != tuple(ids.shape):
        raise RecAttendError('--input %s: x_full is %s %s, expected uint8 [%d,%d,%d,3] (the labels\' size)' % (
            args.input, x_full.dtype, tuple(x_full.shape), ids.shape[0], ids.shape[1], ids.shape[2]))
      x = resize_images(lambda i: x_full[i], ids.shape[0], ids.shape[1:], H, W, args.batch_size)
      orig_size = np.tile(np.asarray(ids.shape[1:], np.int32), (ids.shape[0], 1))
  out = assemble_archive(ids, names, x, args.dataset, H, W, T, args.target, args.batch_size)
  if orig_size is not None:
    out['orig_size'] = orig_size
  folder = os.path.dirname(os.path.abspath(args.output))
  os.makedirs(folder, exist_ok=True)
  np.savez(args.output, **out)
  print('%d images, %d x %d -> %d x %d, timespan %d -> %s (%s)' % (ids.shape[0], ids.shape[1], ids.shape[2], H, W, T, args.output,
                                                                 ', '.join(sorted(out))))
  return out


if __name__ == '__main__':
  main()
