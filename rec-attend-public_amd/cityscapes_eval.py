#!/usr/bin/env python
"""Entry point with the flag surface of the reference's cityscapes_eval.py (:260-272 + EvalArgsParser): the stage BEHIND the
decode loop, which turns decoded instance masks and the pre-stage's semantic map into the Cityscapes instance-level output —
one mask, one class id and one score per instance.

Like the reference it does not run the model.  --input is an .npz with
  y_out_ins [N,T,h,w]   the decoded masks at network size (full_model_eval.py's pred_rank<r>.npz: y_out),
  s_out     [N,T]       their scores ([N,T,K]: channel 0, as full_model_eval.py reads multi-class scores),
  y_out     [N,h,w,C]   the pre-stage's semantic map (fg_model_pack.py's y_out / full_model's y_in; channel 0 = background),
and optionally y_gt_full [N,T,H,W] + s_gt [N,T] (ground truth at the labels' size: the --analyzers then run per threshold),
names (N file names, default 'image_<i>') and full_size (H, W; default: y_gt_full's size, else 1024 x 2048 for
--dataset cityscapes and the network size otherwise), and gt_instance_ids [N,H,W] (the values of the *_gtFine_instanceIds.png files
at full_size: then the Cityscapes instance-level AP is computed as well, see below).

Per image (write_log, :148-205), all on the device, batch by batch:
  1. + 2. the foreground mask of the semantic map at full size, FG_THRESHOLD = 0.3 (ops.sem_foreground);
  3. pp.upsample -> pp.apply_confidence -> pp.apply_one_label, then for every threshold of --threshold_list (default
     0.0 ... 0.9) pp.apply_threshold -> pp.mask_foreground -> pp.remove_tiny(--remove_tiny, default 400).  Two things differ
     from full_model_eval.py's chain and are followed as they stand in the reference: upsample comes BEFORE
     apply_confidence, and `conf` is re-assigned inside the threshold loop (:188-189), so an instance that remove_tiny zeroes
     at one threshold keeps conf = 0 at every later threshold;
  4. the class vote and the pick (analysis.f_instance_class);
  5. <output>/output_<split>/cityscapes/<run>/<name>.txt + one 8-bit PNG per written instance
     (analysis.RenderCityScapesOutputAnalyzer); every threshold writes into the same folder, as in the reference, so the last
     threshold of the list is what remains on disk.
  6. with gt_instance_ids in --input: AP and AP50% of the reference's last step (run_cityscapes_eval.sh:51,
     evalInstanceLevelSemanticLabeling.py) per threshold from the masks on the device (analysis.CityscapesAPAnalyzer), written
     to <output>/output_<split>/resultInstanceLevelSemanticLabeling.json: the script's structure for the LAST threshold — what
     the files left on disk would score — plus a key 'thresholds' with the averages of every threshold.
The per-threshold means of the analyzers go to <output>/output_<split>/metrics.yaml.  Two names of the reference's default
--analyzers list (and of its --test list), fg_iou_all and bg_iou_all, accumulate over the whole dataset (analysis.py:834-900)
and are not built HERE: the default lists run without them and say so on standard output; naming one explicitly is an error
(the two accumulators themselves are analysis.ForegroundIOUAnalyzer / BackgroundIOUAnalyzer, driven by fg_model_eval.py).

--semantic_labels PATH (not a reference flag) names the instances from an EXTERNAL semantic segmentation given as label images,
the reference's --lrr_seg path (:162-164, :212-232) behind any segmenter: PATH is a folder holding one
<city>_<seq>_<frame>*.png of label values per image name (8-bit grey, at full_size), or an .npz with labels uint8 [N,H,W] and
names; --semantic_label_ids labelIds|trainIds|lrr says which values are the eight thing classes (default labelIds).  --input
then need not hold y_out: the one-hot map, its foreground mask ("a thing class") and the vote are integer counting, done for
every threshold from one read of the masks (iter_label_instances_from_labels, csrc/ra_label_vote.hip).  The integer counts
define the class; the reference's float32 means of means equal counts / (H * W) exactly when H and W are powers of two
(1024 x 2048 is) and can otherwise differ only in near-ties of two classes.

--lrr_seg, --foreground_folder and --render_gt are accepted and refused: they read files of the authors' machines (LRR .mat
files, a foreground folder, the HDF5 dataset); --lrr_filename is accepted and unused (its default there is a path of that
cluster).  --render_instances (not a reference flag: the reference's runner always renders, cityscapes_eval.py:67-75) writes per
threshold <output>/output_<split>/<NN>/<name>.png, NN = int(threshold * 100) — every instance of that threshold's y_out in its own
colour, composed on the device (analysis.RenderInstanceAnalyzer) — with s_gt in --input also <NN>/count.csv
(analysis.CountAnalyzer needs the ground-truth count), and with y_gt_full also <output>/output_<split>/gt/<name>.png, the ground
truth coloured by its best-matching prediction of the last threshold (analysis.RenderGroundtruthInstanceAnalyzer; unlike
--render_gt it reads the labels from --input).  --split_id / --num_split select images [split_id * num_split, (split_id + 1) * num_split) (:41-46).  There is no
CPU path: without a GPU the stage raises RecAttendError."""
import argparse
import os

import numpy as np
import yaml

import cmd_args_parser as cap
from ra_native import RecAttendError

FG_THRESHOLD = 0.3  # :171
DEFAULT_ANALYZERS = ['sbd', 'wt_cov', 'unwt_cov', 'fg_dice', 'fg_iou', 'fg_iou_all', 'bg_iou_all', 'avg_fp', 'avg_fn', 'avg_pr',
                     'avg_re', 'obj_pr', 'obj_re', 'count_acc', 'count_mse', 'dic', 'dic_abs']  # :294-298
TEST_ANALYZERS = ['fg_iou', 'fg_iou_all', 'bg_iou_all']  # :292
# whole-dataset foreground / background IoU (analysis.py:834-900): accumulating analyzers, not per-image functions; not built
NOT_BUILT = ('fg_iou_all', 'bg_iou_all')
SEMANTIC_LABEL_IDS = ('labelIds', 'trainIds', 'lrr')  # the keys of ra_ops.LABEL_CLASS_IDS (not imported here: no torch yet)
MAX_BATCH_ELEMS = 1 << 29  # floats of one [B,T,H,W] tensor of the chain (2 GiB); several are alive at a time

REFUSED = {
    'lrr_seg': '--lrr_seg reads the LRR segmentation .mat files of the authors\' cluster (cityscapes_eval.py:207-230); give the '
               'semantic map as y_out in --input instead, or the segmentation as label images with --semantic_labels',
    'foreground_folder': '--foreground_folder reads a folder of foreground images of the authors\' cluster; give the semantic '
                         'map as y_out in --input instead, or a segmentation as label images with --semantic_labels',
    'render_gt': '--render_gt renders the ground truth from the HDF5 dataset, which is out of scope here; --render_instances '
                 'renders it from y_gt_full of --input',
}


def build_parser():
  p = argparse.ArgumentParser(description='Eval ris pp output')
  for table in (cap.CITYSCAPES_EVAL_FLAGS, cap.DATA_FLAGS):
    cap.add_flags(p, table)
  p.add_argument('--input', default=None, help='.npz with y_out_ins [N,T,h,w], s_out [N,T], y_out [N,h,w,C] '
                                               '(+ y_gt_full, s_gt, names, full_size)')
  p.add_argument('--render_instances', action='store_true',
                 help='not a reference flag (the reference always renders): write every threshold\'s instances as a colour image into '
                      '<output>/output_<split>/<NN>/, count.csv beside them when --input has s_gt, and the ground truth coloured by '
                      'its best match into gt/ when it has y_gt_full')
  p.add_argument('--device_png', action='store_true',
                 help='not a reference flag: compress the instance masks and the --render_instances images on the device (a run '
                      'code within each row, utils/png.write_*_dev) instead of copying every plane to the host for zlib; the '
                      'files decode to the same pixels, their bytes differ and they are larger')
  cap.add_device_png_code(p)
  p.add_argument('--semantic_labels', default=None,
                 help='not a reference flag: name the instances from an external semantic segmentation given as label images (the '
                      '--lrr_seg path behind any segmenter): a folder with one <city>_<seq>_<frame>*.png per image name, or an '
                      '.npz with labels uint8 [N,H,W] and names; --input then need not hold y_out')
  p.add_argument('--semantic_label_ids', default='labelIds', choices=SEMANTIC_LABEL_IDS,
                 help='which values of --semantic_labels are the eight thing classes: labelIds 24..28,31..33, trainIds 11..18, '
                      'lrr 12..19 (cityscapes_eval.py:213-216)')
  return p


def make_opt(args):
  """CityscapesEvalArgsParser.make_opt (:274-306)."""
  for flag, why in REFUSED.items():
    if getattr(args, flag):
      raise RecAttendError(why)
  opt = {k: getattr(args, k) for k in ('split_id', 'num_split', 'remove_tiny', 'no_iou', 'output', 'results', 'model_id',
                                        'batch_size', 'dataset')}
  opt['split'] = args.split.split(',')
  opt['threshold_list'] = ([i * 0.1 for i in range(10)] if args.threshold_list is None
                           else [float(t) for t in args.threshold_list.split(',')])
  if args.analyzers is None:
    opt['analyzers'] = [n for n in (TEST_ANALYZERS if args.test else DEFAULT_ANALYZERS) if n not in NOT_BUILT]
    print('analyzers: the default list without %s (whole-dataset accumulators, not built)' % ', '.join(NOT_BUILT))
  else:
    opt['analyzers'] = [n for n in args.analyzers.split(',') if n]
    for n in opt['analyzers']:
      if n in NOT_BUILT:
        raise RecAttendError('analyzer %s accumulates over the whole dataset (analysis.py:834-900) and is not built' % n)
  return opt


def _need_device():
  import torch
  if not torch.cuda.is_available():
    raise RecAttendError('the Cityscapes output stage runs on the GPU; no device is available and there is no CPU fallback')
  return torch


def iter_label_instances(y_ins, s_out, sem, size, thresholds, remove_tiny=400):
  """Steps 1-4 of the module docstring on device tensors: y_ins [B,T,h,w], s_out [B,T] (or [B,T,K]: channel 0), sem
  [B,h',w',C], size = (H, W).  Yields one dict per threshold, in order: 'threshold', 'y_out' [B,T,H,W] binary, 's_out'
  (s_out > 0.5), 'conf' [B,T] (s_out with the instances remove_tiny dropped at this or an EARLIER threshold zeroed),
  'y_in' (sem), 'fg' [B,H,W], 'class_idx', 'label_id' int32 [B,T] (-1 = not written), 'vote' [B,T,C]."""
  torch = _need_device()
  import ra_ops as ops
  from utils import postprocess as pp
  for t in (y_ins, s_out, sem):
    if not t.is_cuda:
      raise RecAttendError('the Cityscapes output stage needs device tensors; there is no CPU fallback')
  H, W = int(size[0]), int(size[1])
  if s_out.dim() == 3:
    s_out = s_out[:, :, 0]
  s_out = s_out.contiguous().to(torch.float32)
  sem = sem.contiguous()
  fg = ops.sem_foreground(sem, H, W, FG_THRESHOLD)            # :166-176
  y = pp.upsample(y_ins.contiguous(), (H, W))                 # :179
  y, conf_hard = pp.apply_confidence(y, s_out)                # :180
  one = pp.apply_one_label(y)                                 # :181
  del y
  conf = s_out.clone()
  for th in thresholds:
    y_bin = pp.mask_foreground(pp.apply_threshold(one, float(th)), fg)                # :184-185
    y_bin, conf = pp.remove_tiny(y_bin, conf, threshold=remove_tiny)                  # :188-189: conf carries over
    vote, idx, lab = ops.instance_class_vote(y_bin, sem, conf)                        # analysis.py:232-261
    yield {'threshold': float(th), 'y_out': y_bin, 's_out': conf_hard, 'conf': conf, 'y_in': sem, 'fg': fg,
           'class_idx': idx, 'label_id': lab, 'vote': vote, '_instance_class': (idx, lab, vote)}


def label_instances(y_ins, s_out, sem, size, thresholds, remove_tiny=400):
  """list(iter_label_instances(...)): every threshold's tensors at once ([B,T,H,W] floats each — mind the size)."""
  return list(iter_label_instances(y_ins, s_out, sem, size, thresholds, remove_tiny))


def iter_label_instances_from_labels(y_ins, s_out, labels, size, thresholds, remove_tiny=400, ids='labelIds', planes=True):
  """iter_label_instances behind an external semantic segmentation given as a label image (the reference's --lrr_seg path,
  :162-164, :212-232): labels uint8 [B,H,W] at size = (H, W), ids the convention of its values (ra_ops.label_class_lut).
  Yields the same keys per threshold, so the analyzers and renderers take it unchanged: 'y_in' is None, 'labels' the label
  image, 'fg' [B,H,W] = "a thing class", 'vote' [B,T,9] = counts / (H * W) with channel 0 zero, and '_instance_class' is
  supplied, so analysis.f_instance_class never calls the resampling vote; also 'sizes' [B,T] and 'counts' [B,T,8] (int32).
  One read of the masks serves every threshold (ops.label_vote_sweep), one read and one write makes a threshold's planes
  (ops.label_planes).  planes=False: 'y_out' is None and only the sweep runs — class, score and size of every instance at
  every threshold, without the masks (the analyzers and renderers need the masks)."""
  torch = _need_device()
  import ra_ops as ops
  from utils import postprocess as pp
  for t in (y_ins, s_out, labels):
    if not t.is_cuda:
      raise RecAttendError('the Cityscapes output stage needs device tensors; there is no CPU fallback')
  H, W = int(size[0]), int(size[1])
  if labels.dtype != torch.uint8 or tuple(labels.shape) != (y_ins.shape[0], H, W):
    raise RecAttendError('labels must be uint8 %s (one label image per example at size), got %s %s'
                         % ((y_ins.shape[0], H, W), labels.dtype, tuple(labels.shape)))
  if s_out.dim() == 3:
    s_out = s_out[:, :, 0]
  s_out = s_out.contiguous().to(torch.float32)
  labels = labels.contiguous()
  lut = ops.label_class_lut(ids)
  fg = (torch.from_numpy(lut).to(labels.device)[labels.long()] > 0).to(torch.float32)  # :164: 1 - onehot[..., 0]
  y = pp.upsample(y_ins.contiguous(), (H, W))                 # :179
  y, conf_hard = pp.apply_confidence(y, s_out)                # :180
  thresholds = [float(th) for th in thresholds]
  conf = s_out
  for k0 in range(0, len(thresholds), ops.LABEL_VOTE_MAX_K):   # conf carries over from one sweep to the next
    part = thresholds[k0:k0 + ops.LABEL_VOTE_MAX_K]
    sw = ops.label_vote_sweep(y, labels, lut, part, conf, remove_tiny)
    conf = sw['conf'][-1]
    for k, th in enumerate(part):
      y_bin = ops.label_planes(y, labels, lut, th, keep=sw['keep'][k]) if planes else None
      idx, lab, vote = sw['class_idx'][k], sw['label_id'][k], sw['vote'][k]
      yield {'threshold': th, 'y_out': y_bin, 's_out': conf_hard, 'conf': sw['conf'][k], 'y_in': None, 'labels': labels, 'fg': fg,
             'class_idx': idx, 'label_id': lab, 'vote': vote, 'sizes': sw['sizes'][k], 'counts': sw['counts'][k],
             '_instance_class': (idx, lab, vote)}


def semantic_label_reader(path, names, size):
  """--semantic_labels: a function i -> the label image uint8 [H,W] of image names[i].  path is a folder searched as
  cityscapes_pixel.find_prediction searches --pred (the one <city>_<seq>_<frame>*.png below it), or an .npz with labels uint8
  [N,H,W] and names.  No match, several matches and a size other than size = (H, W) are errors, raised when the image is
  asked for."""
  H, W = int(size[0]), int(size[1])
  if os.path.isdir(path):
    import fnmatch
    from cityscapes_ap import image_stem
    from utils import png
    walk = [(root, files) for root, _, files in os.walk(path)]

    def read(i):
      name = str(names[i])
      hits = [os.path.join(root, f) for root, files in walk for f in fnmatch.filter(files, image_stem(name) + '*.png')]
      if not hits:
        raise RecAttendError('--semantic_labels: found no label image for %s below %s' % (name, path))
      if len(hits) > 1:
        raise RecAttendError('--semantic_labels: found several label images for %s: %s' % (name, ', '.join(sorted(hits))))
      img = png.read_gray8(hits[0])
      if img.shape != (H, W):
        raise RecAttendError('--semantic_labels: %s is %d x %d, expected full_size %d x %d' % ((hits[0],) + img.shape + (H, W)))
      return img
    return read
  if not os.path.isfile(path):
    raise RecAttendError('--semantic_labels: %s is neither a folder nor an .npz file' % path)
  data = np.load(path, allow_pickle=False)
  for k in ('labels', 'names'):
    if k not in data:
      raise RecAttendError('--semantic_labels %s lacks %s' % (path, k))
  labels, have = data['labels'], [str(n) for n in data['names']]
  if labels.dtype != np.uint8 or labels.ndim != 3 or labels.shape[0] != len(have):
    raise RecAttendError('--semantic_labels %s: labels is %s %s, expected uint8 [N,H,W] for its %d names'
                         % (path, labels.dtype, labels.shape, len(have)))

  def pick(i):
    name = str(names[i])
    hits = [j for j, n in enumerate(have) if n == name]
    if not hits:
      raise RecAttendError('--semantic_labels: %s has no label image for %s' % (path, name))
    if len(hits) > 1:
      raise RecAttendError('--semantic_labels: %s names %s %d times' % (path, name, len(hits)))
    if labels.shape[1:] != (H, W):
      raise RecAttendError('--semantic_labels: %s is %d x %d, expected full_size %d x %d' % ((path,) + labels.shape[1:] + (H, W)))
    return labels[hits[0]]
  return pick


def _full_size(data, dataset):
  if 'full_size' in data:
    return int(data['full_size'][0]), int(data['full_size'][1])
  if 'y_gt_full' in data:
    return tuple(int(v) for v in data['y_gt_full'].shape[-2:])
  if dataset == 'cityscapes':
    return 1024, 2048
  return tuple(int(v) for v in data['y_out_ins'].shape[-2:])


def main(argv=None):
  args = build_parser().parse_args(argv)
  png_code = cap.device_png_code(args)
  opt = make_opt(args)
  if args.input is None:
    raise RecAttendError('--input is required: an .npz with y_out_ins, s_out and y_out (the stage does not run the model)')
  if opt['output'] is None:
    if args.model_id is None:
      raise Exception('You must provide model ID')  # cmd_args_parser.py:154-155 (needed for the default output folder)
    opt['output'] = os.path.join(args.results, args.model_id)  # CityscapesEvalExperiment.get_runner :236-239
  torch = _need_device()
  import analysis
  data = dict(np.load(args.input, allow_pickle=False))
  for k in ('y_out_ins', 's_out') + (() if args.semantic_labels else ('y_out',)):
    if k not in data:
      raise RecAttendError('--input lacks %s' % k)
  N, T = data['y_out_ins'].shape[:2]
  H, W = _full_size(data, args.dataset)
  names = [str(n) for n in data['names']] if 'names' in data else ['image_%06d' % i for i in range(N)]
  lo, hi = (0, N) if opt['split_id'] == -1 else (min(N, opt['split_id'] * opt['num_split']),
                                                min(N, (opt['split_id'] + 1) * opt['num_split']))  # :41-46
  read_labels = semantic_label_reader(args.semantic_labels, names, (H, W)) if args.semantic_labels else None
  have_gt = 'y_gt_full' in data and 's_gt' in data
  an_names = opt['analyzers'] if have_gt else []
  out_dir = os.path.join(opt['output'], 'output_' + opt['split'][0])
  os.makedirs(out_dir, exist_ok=True)
  thresholds = opt['threshold_list']
  dpng = bool(getattr(args, 'device_png', False))
  renders = [analysis.RenderCityScapesOutputAnalyzer(os.path.join(out_dir, 'cityscapes'), names, device_png=dpng, device_png_code=png_code)
             for _ in thresholds]
  have_ids = 'gt_instance_ids' in data
  all_ids = data['gt_instance_ids'] if have_ids else None  # the largest array of the file: inflated once, not once per batch
  if have_ids and tuple(all_ids.shape) != (N, H, W):
    raise RecAttendError('--input: gt_instance_ids is %s, expected %s (N images at full_size)' % (tuple(all_ids.shape), (N, H, W)))
  scorers = [analysis.CityscapesAPAnalyzer(names) for _ in thresholds] if have_ids else []
  acc = [{n: [] for n in an_names} for _ in thresholds]
  img_render, counters, gt_render, have_y_gt = [], [], None, 'y_gt_full' in data
  if args.render_instances:
    folders = [os.path.join(out_dir, '{:02d}'.format(int(th * 100))) for th in thresholds]  # cityscapes_eval.py:65
    img_render = [analysis.RenderInstanceAnalyzer(f, names, device_png=dpng, device_png_code=png_code) for f in folders]
    if 's_gt' in data:
      counters = [analysis.CountAnalyzer(os.path.join(f, 'count.csv')) for f in folders]
    else:
      print('--render_instances: no count.csv, --input has no s_gt to count against')
    if have_y_gt:
      gt_render = analysis.RenderGroundtruthInstanceAnalyzer(os.path.join(out_dir, 'gt'), names, device_png=dpng,
                                                                   device_png_code=png_code)
  bs = max(1, min(opt['batch_size'], MAX_BATCH_ELEMS // max(1, T * H * W)))
  dev = torch.device('cuda', torch.cuda.current_device())
  up = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
  for b0 in range(lo, hi, bs):
    b1 = min(hi, b0 + bs)
    gt = up(data['y_gt_full'][b0:b1]) if have_gt or gt_render is not None else None
    sg = up(data['s_gt'][b0:b1]) if have_gt or counters else None
    ids = torch.as_tensor(np.ascontiguousarray(all_ids[b0:b1], dtype=np.int32)).to(dev) if have_ids else None
    if read_labels is not None:
      seg = torch.from_numpy(np.stack([read_labels(i) for i in range(b0, b1)])).to(dev)
      chain = iter_label_instances_from_labels(up(data['y_out_ins'][b0:b1]), up(data['s_out'][b0:b1]), seg, (H, W), thresholds,
                                               opt['remove_tiny'], ids=args.semantic_label_ids)
    else:
      chain = iter_label_instances(up(data['y_out_ins'][b0:b1]), up(data['s_out'][b0:b1]), up(data['y_out'][b0:b1]), (H, W),
                                   thresholds, opt['remove_tiny'])
    for tt, res in enumerate(chain):
      res['indices'] = list(range(b0, b1))
      if have_gt:
        res['y_gt'], res['s_gt'] = gt, sg
        if not opt['no_iou']:
          res['iou_pairwise'] = analysis.f_iou_pairwise(res['y_out'], gt)  # :199-202
        for n in an_names:
          acc[tt][n].append(analysis.create_analyzer(n)(res).cpu().numpy())
      renders[tt].stage(res)
      if img_render:
        img_render[tt].stage(res)
        if counters:
          counters[tt].stage(dict(res, s_gt=sg))
        if gt_render is not None and tt == len(thresholds) - 1:  # after the last threshold, as full_model_eval.py:139-140
          iou = res['iou_pairwise'] if 'iou_pairwise' in res else analysis.f_iou_pairwise(res['y_out'], gt)
          gt_render.stage({'y_gt': gt, 'iou_pairwise': iou, 'indices': res['indices']})
      if have_ids:
        res['gt_ids'] = ids
        scorers[tt].stage(res)
  for r in renders:
    r.finalize()
  summary = {}
  for tt, th in enumerate(thresholds):
    vals = {n: np.concatenate(v) if v else np.zeros(0) for n, v in acc[tt].items()}
    summary['%.2f' % th] = {n: {'mean': float(v.mean()) if v.size else 0.0, 'count': int(v.size)} for n, v in vals.items()}
  with open(os.path.join(out_dir, 'metrics.yaml'), 'w') as f:
    yaml.safe_dump(summary, f)
  if have_ids:
    import json
    results = [sc.finalize(quiet=True) for sc in scorers]
    out = dict(results[-1], thresholds={'%.2f' % th: r['averages'] for th, r in zip(thresholds, results)})
    with open(os.path.join(out_dir, 'resultInstanceLevelSemanticLabeling.json'), 'w') as f:
      json.dump(out, f, indent=4, sort_keys=True)
    print(analysis.cityscapes_ap_table(out['averages']))
  print('images [%d, %d) -> %s' % (lo, hi, os.path.join(out_dir, 'cityscapes')))
  return renders


if __name__ == '__main__':
  main()
