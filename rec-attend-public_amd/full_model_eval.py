#!/usr/bin/env python
"""Entry point with the flag surface of the reference's full_model_eval.py (:180-222).

Restores results/<model_id>/{model_opt.yaml, weights.npz}, forces `use_knob=False`
(full_model_eval.py:172-174), feeds {x, phase_train=False[, d_in, y_in]} and fetches
['y_out', 's_out'] (full_model_eval.py:35; runner.py:91-105) batch by batch on the MI355X
kernels, sharding the images over the ranks when launched with torch.distributed.run.  Inputs
come from --input (an .npz with x [N,H,W,3] and optionally d_in / y_in / y_gt / s_gt / fg / gt_instance_ids / names) or are
synthetic; with --fg_model_id (not a reference flag) d_in / y_in come from that fg_model's prestage() on the device, batch by
batch, as the 8-bit values fg_model_pack.py would store; the reference's HDF5 datasets are out of scope.  The raw outputs are
written to <output>/output_<split>/pred_rank<r>.npz.  With y_gt and s_gt in the input the
reference's write_log chain (full_model_eval.py:97-139) runs on the device for every threshold of
--threshold_list (default 0.3, the reference CLI's default, :193-194): apply_confidence, apply_one_label,
apply_threshold [, mask_foreground, remove_tiny] and the --analyzers (default list :201-205);
the per-threshold means go to <output>/output_<split>/metrics_rank<r>.yaml.  The cv2 steps
(upsample + bilateral filter, morph) run as device kernels (utils/postprocess.py).  As in the reference, pp.upsample — cv2.resize
to the labels' size, then bilateralFilter(5, 10, 10), which on [0, 1] maps is close to a radius-2 blur — ALWAYS runs, also when
the labels already have the network's size (full_model_eval.py:114), and the dilation runs when a foreground mask is given and
--no_morph is not.  --fused_postprocess (not a reference flag) skips the bilateral step when no resize is needed: the chain
then collapses into one fused device pass; masks and metrics near the threshold differ from the reference's in that mode.
The labels may instead be instance-id images: an --input with gt_instance_ids [N,Hf,Wf] (integers, what setup_labels.py reads)
and NO y_gt evaluates at the labels' own size without ever holding a [T,Hf,Wf] float plane.  Per batch ops.assemble_labels at
network size, under the --dataset rule, gives the slots' ids (the reference's order, by area at network size) and s_gt — an
image it cannot take is reported by its name of `names` — and behind apply_confidence the whole chain is ONE counting pass for
all thresholds (ops.instance_eval_counts: resize + bilateral filter, the dilation when a foreground is given and --no_morph is
not, first maximum, threshold, foreground mask) whose integers ops.eval_metrics_from_counts turns into what every analyzer
reads; --remove_tiny acts on the counted areas where a foreground is given, as in the chain.  fg, optional, is then a 0 / 1
mask [N,Hf,Wf]; another value is an error naming the image.  metrics_rank<r>.yaml has the same format on both paths.  The
thresholds must be >= 0 there.  --render and --render_gt_instances draw the thresholded masks, which this path never writes,
and --fused_postprocess has nothing to skip on it: all three are refused by name.  An archive that holds y_gt takes the plane
path, whatever else it holds.  Mixed full sizes (KITTI): an --input with gt_instance_ids_flat [P], pixel_offset [N + 1] and
orig_size [N,2] (what setup_labels.py --mixed_sizes writes) and no y_gt takes the same id path through the ragged entry points
(ops.assemble_labels_ragged, ops.instance_eval_counts_ragged): every batch is still ONE launch chain, each image resized,
filtered and counted at its own size; an optional fg_flat uint8 [P] is the 0 / 1 foreground at the same offsets.  On such an
archive --render, --render_gt_instances, --fused_postprocess and --cityscapes_output are refused by name.
--cityscapes_output DIR (not a reference flag; needs --fg_model_id with a 9-class pre-stage) puts the reference's THIRD stage
behind the loop: every decoded batch and the pre-stage's y_in go through cityscapes_eval.label_instances on the device — its
chain, not the one above: upsample before apply_confidence, the semantic map's own foreground mask, conf carried across the
thresholds — at --threshold_list / --remove_tiny, and DIR/<run>/<name>.txt + one PNG per written instance come out
(analysis.RenderCityScapesOutputAnalyzer; the labels' size is y_gt's or full_size's of --input, else the network's; file
names from `names` of --input, else image_<index>).  pred_rank<r>.npz is the same with and without the flag.
--render (not a reference flag; the reference's runner always renders, full_model_eval.py:170) writes what the write_log chain
ends in there: per threshold <output>/output_<split>/<NN>/<name>.png, NN = int(threshold * 100) (:65) — every instance of the
chain's thresholded masks in its own colour, composed on the device (analysis.RenderInstanceAnalyzer) — and <NN>/count.csv
(analysis.CountAnalyzer); --render_gt_instances adds <output>/output_<split>/gt/<name>.png, the ground truth coloured by its
best-matching prediction of the LAST threshold (:139-140, analysis.RenderGroundtruthInstanceAnalyzer).  Both need y_gt and s_gt in
--input, where the chain runs.  With several ranks each rank writes the images of its shard and its counts go to
<NN>/count_rank<r>.csv.
--render_from_ids / --render_gt_from_ids (not reference flags) write the same files on the id path, uniform and mixed sizes,
where no mask exists: the counting pass also returns its winner map — uint16 per full-size pixel, the prediction that holds
it and how many of the thresholds it passes: every thresholded mask of every threshold at once — requested once per group of
up to 16 thresholds, and ops.paint_instances looks the pictures up from it behind ops.eval_metrics_from_counts, whose areas
say which predictions --remove_tiny took; the ground truth is painted from the id image (ops.paint_groundtruth) in
analysis.groundtruth_colours of the last threshold's iou_pairwise.  Both honour --device_png / --device_png_code (a batch of
mixed sizes is encoded where it lies, in one launch chain: analysis.RaggedPicture, ops.png_deflate_ragged).  Off the id path
each is refused by name and points to --render / --render_gt_instances, whose refusals on id and mixed-size archives stay as
they are."""
import argparse
import os
import time

import numpy as np
import yaml

import cmd_args_parser as cap
import full_model
import ra_dist


def build_parser():
  p = argparse.ArgumentParser(description='Evaluate output')
  for table in (cap.EVAL_FLAGS, cap.DATA_FLAGS):
    cap.add_flags(p, table)
  p.add_argument('--input', default=None, help='.npz with x [N,H,W,3] (+ d_in, y_in)')
  p.add_argument('--num_synthetic', type=int, default=8)
  p.add_argument('--fused_postprocess', action='store_true',
                 help='not a reference flag: skip upsample\'s bilateral filter when the labels have the network\'s size (one fused '
                      'post-processing pass; results near the threshold differ from the reference chain)')
  p.add_argument('--fg_model_id', default=None,
                 help='not a reference flag: run this fg_model (results/<id>/{model_opt.yaml, weights.npz}) in front of the decode '
                      'loop; d_in / y_in then come from its prestage() on the device, not from --input')
  p.add_argument('--cityscapes_output', default=None,
                 help='not a reference flag: write the Cityscapes instance-level output (a mask, a class id and a score per instance) '
                      'of every decoded image into this folder; needs --fg_model_id with 9 semantic classes')
  p.add_argument('--render', action='store_true',
                 help='not a reference flag (the reference always renders): write every thresholded output as a colour image, one '
                      'colour per instance, and count.csv into <output>/output_<split>/<NN>/; needs y_gt and s_gt in --input')
  p.add_argument('--render_gt_instances', action='store_true',
                 help='not a reference flag: write the ground truth, coloured by its best-matching prediction, into '
                      '<output>/output_<split>/gt/; needs y_gt and s_gt in --input')
  p.add_argument('--render_from_ids', action='store_true',
                 help='not a reference flag: what --render writes (<NN>/<name>.png per threshold and <NN>/count.csv), on an --input '
                      'that holds gt_instance_ids (or the flat layout of mixed sizes) and no y_gt: painted from the counting pass\'s '
                      'winner map, 2 bytes per pixel, so no [T,Hf,Wf] plane is held; the pictures themselves are 3 bytes per pixel and '
                      'threshold on the device at a time (503 MB at --batch_size 8, 1024 x 2048 and ten thresholds)')
  p.add_argument('--render_gt_from_ids', action='store_true',
                 help='not a reference flag: what --render_gt_instances writes (gt/<name>.png), on the same kind of --input: painted '
                      'from the id images')
  p.add_argument('--device_png', action='store_true',
                 help='not a reference flag: compress the files of --render, --render_gt_instances and --cityscapes_output on the '
                      'device (a run code within each row, utils/png.write_*_dev) instead of copying every plane to the host for '
                      'zlib; the files decode to the same pixels, their bytes differ and they are larger')
  cap.add_device_png_code(p)
  p.add_argument('--in_flight', type=int, default=8, help='batches submitted to one GPU at a time (four decode concurrently, the rest queue behind them)')
  return p


FLAT_KEYS = ('gt_instance_ids_flat', 'pixel_offset', 'orig_size')


def _flat_path(keys):
  """The labels of --input are instance-id images of mixed full sizes in the flat layout, and no y_gt."""
  return all(k in keys for k in FLAT_KEYS) and 'y_gt' not in keys


def _id_path(keys):
  """The labels of --input are instance-id images: gt_instance_ids [N,Hf,Wf], or the flat layout of mixed sizes, and no y_gt
  (an archive with y_gt keeps the plane path it always took)."""
  return ('gt_instance_ids' in keys or _flat_path(keys)) and 'y_gt' not in keys


def main(argv=None):
  import torch
  args = build_parser().parse_args(argv)
  cap.device_png_code(args)  # refused here, before any work, when it comes without --device_png
  if args.model_id is None:
    raise Exception('You must provide model ID')  # cmd_args_parser.py:154-155
  if args.cityscapes_output and not args.fg_model_id:
    from ra_native import RecAttendError
    raise RecAttendError('--cityscapes_output needs --fg_model_id: the instance classes are voted on the pre-stage\'s semantic map')
  from_ids = [f for f, on in (('--render_from_ids', args.render_from_ids), ('--render_gt_from_ids', args.render_gt_from_ids)) if on]
  if from_ids:  # the id path's own render flags: refused by name wherever that path does not run
    from ra_native import RecAttendError
    if not args.input:
      raise RecAttendError('%s needs --input with gt_instance_ids (or the flat layout of mixed sizes) and no y_gt: it paints from '
                           'the id path\'s counting pass, and synthetic input has no labels; with y_gt and s_gt in --input use '
                           '--render / --render_gt_instances' % ' / '.join(from_ids))
    with np.load(args.input) as peek:
      on_id_path = _id_path(peek.files)
    if not on_id_path:
      raise RecAttendError('%s cannot be used with an --input that takes the plane path (%s holds y_gt, or no gt_instance_ids): '
                           'it paints from the id path\'s counting pass; use --render / --render_gt_instances there' % (
                               ' / '.join(from_ids), args.input))
  if args.input:  # before anything is restored: what the id path cannot do is refused by name
    with np.load(args.input) as peek:
      id_path, flat_path = _id_path(peek.files), _flat_path(peek.files)
    if flat_path:
      for f, on in (('--render', args.render), ('--render_gt_instances', args.render_gt_instances),
                    ('--fused_postprocess', args.fused_postprocess), ('--cityscapes_output', args.cityscapes_output)):
        if on:
          from ra_native import RecAttendError
          raise RecAttendError(
              '%s cannot be used with an --input of mixed full sizes (%s holds gt_instance_ids_flat): the images are counted at '
              'their own sizes in one pass that writes no mask, and the render and Cityscapes stages take one size per call' % (
                  f, args.input))
    refused = [f for f, on in (('--render', args.render), ('--render_gt_instances', args.render_gt_instances),
                               ('--fused_postprocess', args.fused_postprocess)) if on]
    if id_path and refused:
      from ra_native import RecAttendError
      raise RecAttendError(
          '%s cannot be used with an --input that holds gt_instance_ids and no y_gt (%s): from id images the write_log chain runs '
          'as one counting pass that never writes the thresholded masks --render / --render_gt_instances draw, and that always '
          'upsamples, so --fused_postprocess has nothing to skip; put y_gt and s_gt into --input for these flags' % (
              ' / '.join(refused), args.input))
  if args.render or args.render_gt_instances:  # the flags render the write_log chain's masks
    from ra_native import RecAttendError
    flags = ' / '.join(f for f, on in (('--render', args.render), ('--render_gt_instances', args.render_gt_instances)) if on)
    if not args.input:
      raise RecAttendError('%s needs --input with y_gt and s_gt: the write_log chain, whose masks it renders, runs on labelled '
                           'input only, and synthetic input has no labels' % flags)
    with np.load(args.input) as peek:
      missing = [k for k in ('y_gt', 's_gt') if k not in peek.files]
    if missing:
      raise RecAttendError('%s needs y_gt and s_gt in --input (the write_log chain, whose masks it renders, runs on labelled '
                           'input only): %s lacks %s' % (flags, args.input, ' and '.join(missing)))
  restore = os.path.join(args.results, args.model_id)
  with open(os.path.join(restore, 'model_opt.yaml')) as f:
    model_opt = yaml.safe_load(f)
  model_opt['use_knob'] = False
  rank, world, local_rank = ra_dist.init()
  if torch.cuda.is_available():
    torch.cuda.set_device(local_rank)
  model = full_model.get_model(model_opt).load_weights(dict(np.load(os.path.join(restore, 'weights.npz'))))
  H, W = model_opt['inp_height'], model_opt['inp_width']
  if args.input:
    data = dict(np.load(args.input))
  else:
    rng = np.random.RandomState(1234)
    data = {'x': rng.rand(args.num_synthetic, H, W, 3).astype(np.float32)}
    if model.dims['add_d_out']:
      n = args.num_synthetic
      data['d_in'] = np.eye(8, dtype=np.float32)[rng.randint(0, 8, (n, H, W))]
      lg = rng.randn(n, H, W, model.dims['nsc']).astype(np.float32)
      data['y_in'] = np.exp(lg) / np.exp(lg).sum(-1, keepdims=True)
  fg = None
  if args.fg_model_id:
    import fg_model_pack
    fg = fg_model_pack.restore_model(args.results, args.fg_model_id)
    for k in ('d_in', 'y_in'):
      data.pop(k, None)
    if args.cityscapes_output and fg.dims['nsc'] != 9:
      from ra_native import RecAttendError
      raise RecAttendError('--cityscapes_output needs a pre-stage with 9 semantic classes (background + the 8 Cityscapes instance '
                           'classes); fg_model %s has %d' % (args.fg_model_id, fg.dims['nsc']))
  lo, hi = ra_dist.shard_range(rank, world, data['x'].shape[0])
  # the reference CLI defaults to [0.3] (MyEvalArgsParser.make_opt, full_model_eval.py:193-198); the
  # 0.0 .. 0.9 sweep of :39-40 is only EvalRunner's fallback for a caller that hands it None
  thresholds = [float(t) for t in args.threshold_list.split(',')] if args.threshold_list else [0.3]
  if args.analyzers is None:                                          # :199-210
    names = [] if args.test else ['sbd', 'wt_cov', 'unwt_cov', 'avg_fp', 'avg_fn', 'avg_pr', 'avg_re',
                                  'obj_pr', 'obj_re', 'count_acc', 'count_mse', 'dic', 'dic_abs']
  else:
    names = [n for n in args.analyzers.split(',') if n]
  want_render = args.render or args.render_gt_instances
  analyze = (bool(names) or want_render) and 'y_gt' in data and 's_gt' in data
  if (bool(names) or bool(from_ids)) and _id_path(data):
    analyze = True
    _check_id_labels(args, data, model)
  acc = {th: {n: [] for n in names} for th in thresholds}
  ys, ss, t0 = [], [], time.time()
  try:
    _run_shard(args, model, data, lo, hi, rank, restore, thresholds, names, analyze, acc, ys, ss, t0, fg=fg, world=world)
  finally:
    ra_dist.barrier()  # always reached: a rank that fails must not leave the others hanging


def _image_names(data):
  return [str(n) for n in data['names']] if 'names' in data else ['image_%06d' % i for i in range(data['x'].shape[0])]


def _check_id_labels(args, data, model):
  """The id path's input, checked on the host before the first batch is decoded."""
  from ra_native import RecAttendError
  import ra_ops as ops
  n = data['x'].shape[0]
  if _flat_path(data):
    import setup_labels
    ids = data['gt_instance_ids_flat']
    if not np.issubdtype(ids.dtype, np.integer):
      raise RecAttendError('--input %s: gt_instance_ids_flat must hold integers, got %s' % (args.input, ids.dtype))
    setup_labels.check_flat('--input %s' % args.input, ids, data['pixel_offset'], data['orig_size'], n)
    ops.label_dataset_rule(args.dataset)
    if 'fg_flat' in data:
      fg, off, size, names = data['fg_flat'], data['pixel_offset'], data['orig_size'], _image_names(data)
      if fg.shape != ids.shape:
        raise RecAttendError('--input %s: fg_flat must be a 0 / 1 mask %s at the ids\' offsets, got %s' % (args.input, ids.shape, fg.shape))
      for i in range(n):
        if not np.isin(fg[off[i]:off[i] + int(size[i, 0]) * int(size[i, 1])], (0, 1)).all():
          raise RecAttendError('--input %s: fg_flat of image %s holds values other than 0 and 1' % (args.input, names[i]))
    return
  ids = data['gt_instance_ids']
  if ids.ndim != 3 or ids.shape[0] != n or not np.issubdtype(ids.dtype, np.integer):
    raise RecAttendError('--input %s: gt_instance_ids must be integers [N,Hf,Wf] with N = %d images (one full size per archive), '
                         'got %s %s' % (args.input, n, ids.dtype, ids.shape))
  ops.label_dataset_rule(args.dataset)
  if 'fg' in data:
    fg, names = data['fg'], _image_names(data)
    if fg.shape != ids.shape:
      raise RecAttendError('--input %s: fg must be a 0 / 1 mask %s at the labels\' size, got %s' % (args.input, ids.shape, fg.shape))
    for i in range(n):
      if not np.isin(fg[i], (0, 1)).all():
        raise RecAttendError('--input %s: fg of image %s holds values other than 0 and 1' % (args.input, names[i]))


def _analyze_ids(args, model, data, b0, b1, y_dev, s_dev, thresholds, names, acc, render=None):
  """The write_log chain (full_model_eval.py:97-139) of one batch from instance-id images: apply_confidence at network size,
  then ONE counting pass at the labels' size for all thresholds (ops.instance_eval_counts) and the analyzers' numbers from
  the counts (ops.eval_metrics_from_counts), handed to analysis through the cache analysis._m honours.  render: the analyzers
  of --render_from_ids / --render_gt_from_ids, {'img': {th: analyzer}, 'count': {th: analyzer}, 'gt': analyzer or None}."""
  import torch
  import ra_ops as ops
  dev = y_dev.device
  if render is not None:
    render = dict(render, indices=list(range(b0, b1)))
  if _flat_path(data):  # mixed full sizes: the same chain through the ragged entry points, one launch chain per batch
    import analysis
    import setup_labels
    off, size = data['pixel_offset'], data['orig_size']
    p0, p1 = int(off[b0]), int(off[b1])
    geo = setup_labels.flat_geometry(off, size, b0, b1)
    ids = torch.as_tensor(np.ascontiguousarray(np.asarray(data['gt_instance_ids_flat'][p0:p1]).astype(np.int32))).to(dev)
    lab = ops.assemble_labels_ragged(ids, geo, model.dims['H'], model.dims['W'], model.dims['T'], args.dataset,
                                     want=('inst_id', 's_gt'), names=_image_names(data)[b0:b1])
    fg = torch.as_tensor(np.ascontiguousarray(np.asarray(data['fg_flat'][p0:p1]).astype(np.uint8))).to(dev) if 'fg_flat' in data else None
    count = lambda yc, ths, want_map=False: ops.instance_eval_counts_ragged(
        yc, ids, geo, lab['inst_id'], ths, fg_flat=fg, morph=fg is not None and not args.no_morph, check_fg=False, want_map=want_map)
    paint = {'instances': lambda wmap, ths, keep: ops.paint_instances(wmap, ths, keep=keep, geo=geo),
             'gt': lambda colours: ops.paint_groundtruth(ids, lab['inst_id'], colours, geo=geo),
             'views': lambda pic: analysis.RaggedPicture(pic, geo)}
    return _analyze_counts(args, count, lab, fg, y_dev, s_dev, thresholds, names, acc, paint, render)
  ids = torch.as_tensor(np.ascontiguousarray(np.asarray(data['gt_instance_ids'][b0:b1]).astype(np.int32))).to(dev)
  # the slots in the reference's order — by area at NETWORK size — under the --dataset rule, as setup_labels.py assembles them
  lab = ops.assemble_labels(ids, model.dims['H'], model.dims['W'], model.dims['T'], args.dataset, want=('inst_id', 's_gt'),
                            names=_image_names(data)[b0:b1])
  fg = torch.as_tensor(np.ascontiguousarray(np.asarray(data['fg'][b0:b1]).astype(np.uint8))).to(dev) if 'fg' in data else None
  count = lambda yc, ths, want_map=False: ops.instance_eval_counts(
      yc, ids, lab['inst_id'], ths, fg=fg, morph=fg is not None and not args.no_morph, check_fg=False, want_map=want_map)
  paint = {'instances': lambda wmap, ths, keep: ops.paint_instances(wmap, ths, keep=keep),
           'gt': lambda colours: ops.paint_groundtruth(ids, lab['inst_id'], colours),
           'views': lambda pic: pic}
  _analyze_counts(args, count, lab, fg, y_dev, s_dev, thresholds, names, acc, paint, render)


def _analyze_counts(args, count, lab, fg, y_dev, s_dev, thresholds, names, acc, paint=None, render=None):
  """apply_confidence, count(yc, thresholds) -> (inter, area_b) in groups of INS_EVAL_MAX_K thresholds, and the analyzers.  With
  render['img'] the counting pass also returns its winner map, once per group, and the group's pictures are painted from it
  behind eval_metrics_from_counts, whose areas say which predictions remove_tiny took: picture and metrics cannot disagree.
  render['gt']: the ground truth painted from the id image in groundtruth_colours of the LAST threshold's iou_pairwise
  (:139-140).  Nothing of size T * Hf * Wf exists on this route."""
  import analysis
  import ra_ops as ops
  from utils import postprocess as pp
  import torch
  s2 = s_dev[:, :, 0].contiguous() if s_dev.dim() == 3 else s_dev   # multi-class: :108-110
  yc, s_conf = pp.apply_confidence(y_dev, s2)
  pictures_wanted = bool(render and render['img'])
  met = None
  for k0 in range(0, len(thresholds), ops.INS_EVAL_MAX_K):
    ths = thresholds[k0:k0 + ops.INS_EVAL_MAX_K]
    if pictures_wanted:
      inter, area_b, wmap = count(yc.contiguous(), ths, True)
    else:
      inter, area_b = count(yc.contiguous(), ths)
    # remove_tiny only where a foreground is given, as in the chain (:121-124)
    per = ops.eval_metrics_from_counts(inter, area_b, lab['s_gt'], remove_tiny=args.remove_tiny if fg is not None else 0, conf=s_conf)
    pictures = paint['instances'](wmap, ths, ops.paint_keep(per)) if pictures_wanted else None
    for k, (th, met) in enumerate(zip(ths, per)):
      results = {'_metrics': met, 'iou_pairwise': met['iou_pairwise'], 's_out': met['conf'], 's_gt': lab['s_gt']}
      for n in names:
        acc[th][n].append(analysis.create_analyzer(n)(results).cpu().numpy())
      if pictures_wanted:  # :71-79: the instance image and the count file of this threshold
        results['indices'], results['picture'] = render['indices'], paint['views'](pictures[k])
        render['img'][th].stage(results)
        render['count'][th].stage(results)
  if render and render['gt'] is not None:
    rgb = analysis.groundtruth_colours(met['iou_pairwise'])
    bgr = torch.as_tensor(np.ascontiguousarray(rgb[:, :, ::-1])).to(y_dev.device)  # the picture's memory order
    render['gt'].stage({'picture': paint['views'](paint['gt'](bgr)), 'indices': render['indices']})


def _run_shard(args, model, data, lo, hi, rank, restore, thresholds, names, analyze, acc, ys, ss, t0, fg=None, world=1):
  import torch
  out_dir = os.path.join(args.output or restore, 'output_' + args.split.split(',')[0])
  img_render, counters, gt_render = {}, {}, None
  dpng, png_code = bool(getattr(args, 'device_png', False)), cap.device_png_code(args)
  # --render_from_ids / --render_gt_from_ids: the same analyzers and the same files, fed by the id path (main has checked that
  # the input takes it)
  ids_img, ids_gt = bool(getattr(args, 'render_from_ids', False)), bool(getattr(args, 'render_gt_from_ids', False))
  if getattr(args, 'render', False) or getattr(args, 'render_gt_instances', False) or ids_img or ids_gt:
    import analysis
    img_names = [str(n) for n in data['names']] if 'names' in data else ['image_%06d' % i for i in range(data['x'].shape[0])]
    if args.render or ids_img:
      for th in thresholds:
        folder = os.path.join(out_dir, '{:02d}'.format(int(th * 100)))  # full_model_eval.py:65
        img_render[th] = analysis.RenderInstanceAnalyzer(folder, img_names, device_png=dpng, device_png_code=png_code)
        counters[th] = analysis.CountAnalyzer(os.path.join(folder, 'count.csv' if world == 1 else 'count_rank%d.csv' % rank))
    if args.render_gt_instances or ids_gt:
      gt_render = analysis.RenderGroundtruthInstanceAnalyzer(os.path.join(out_dir, 'gt'), img_names, device_png=dpng,
                                                                   device_png_code=png_code)
  ids_render = {'img': img_render, 'count': counters, 'gt': gt_render} if ids_img or ids_gt else None
  cs_dir, sems, render = getattr(args, 'cityscapes_output', None), {}, None
  if cs_dir:
    import analysis
    import cityscapes_eval
    n_all = data['x'].shape[0]
    render = analysis.RenderCityScapesOutputAnalyzer(
        cs_dir, [str(n) for n in data['names']] if 'names' in data else ['image_%06d' % i for i in range(n_all)], device_png=dpng,
        device_png_code=png_code)
    if 'full_size' in data:
      cs_size = (int(data['full_size'][0]), int(data['full_size'][1]))
    else:
      cs_size = tuple(int(v) for v in data['y_gt'].shape[-2:]) if 'y_gt' in data else (model.dims['H'], model.dims['W'])

  def consume(b0, b1, y_dev, s_dev):
    if cs_dir:  # the stage behind the loop, on the device: one staging per threshold, as cityscapes_eval.py does
      for res in cityscapes_eval.iter_label_instances(y_dev, s_dev, sems.pop(b0), cs_size, thresholds, args.remove_tiny):
        res['indices'] = list(range(b0, b1))
        render.stage(res)
    if analyze and _id_path(data):
      _analyze_ids(args, model, data, b0, b1, y_dev, s_dev, thresholds, names, acc, render=ids_render)
    elif analyze:
      import analysis
      from utils import postprocess as pp
      dev = y_dev.device
      gt = torch.as_tensor(np.asarray(data['y_gt'][b0:b1], dtype=np.float32)).to(dev)
      sg = torch.as_tensor(np.asarray(data['s_gt'][b0:b1], dtype=np.float32)).to(dev)
      fg = torch.as_tensor(np.asarray(data['fg'][b0:b1], dtype=np.float32)).to(dev) if 'fg' in data else None
      # the reference's chain (full_model_eval.py:112-124): apply_confidence -> upsample to the labels' size (ALWAYS: resize +
      # bilateral filter, also at equal size) -> [foreground given: morph unless --no_morph] -> apply_one_label -> per threshold:
      # apply_threshold [-> mask_foreground -> remove_tiny].  --fused_postprocess: without a resize and a dilation the chain
      # collapses into ONE fused pass (pp.postprocess) that leaves the bilateral step out
      resize = tuple(gt.shape[-2:]) != tuple(y_dev.shape[-2:]) or not getattr(args, 'fused_postprocess', False)
      dilate = fg is not None and not args.no_morph
      if resize or dilate:
        s2 = s_dev[:, :, 0].contiguous() if s_dev.dim() == 3 else s_dev   # multi-class: :108-110
        yc, s_conf = pp.apply_confidence(y_dev, s2)
        if resize:
          yc = pp.upsample(yc, gt)
        if dilate:
          yc = pp.morph(yc)
        one = pp.apply_one_label(yc)
      for th in thresholds:
        if resize or dilate:
          y_bin, s_hard = pp.apply_threshold(one, th), s_conf
          if fg is not None:
            y_bin, s_hard = pp.remove_tiny(pp.mask_foreground(y_bin, fg), s_hard, threshold=args.remove_tiny)
        else:
          y_bin, s_hard, _ = pp.postprocess(y_dev, s_dev, th, fg=fg, remove_tiny_threshold=args.remove_tiny)
        results = {'y_out': y_bin, 'y_gt': gt, 's_out': s_hard, 's_gt': sg}
        for n in names:
          acc[th][n].append(analysis.create_analyzer(n)(results).cpu().numpy())
        if th in img_render:  # :71-79: the instance image and the count file of this threshold
          results['indices'] = list(range(b0, b1))
          img_render[th].stage(results)
          counters[th].stage(results)
      if gt_render is not None:  # :139-140: after the last threshold, with its iou_pairwise
        results['indices'] = list(range(b0, b1))
        gt_render.stage(results)
    ys.append(y_dev if isinstance(y_dev, np.ndarray) else y_dev.cpu().numpy())  # to_host: already host arrays
    ss.append(s_dev if isinstance(s_dev, np.ndarray) else s_dev.cpu().numpy())

  # batches are independent: keep several in flight, each on its own HIP stream, so that the
  # latency-bound tail of one decodes under the controller CNN of the others (DecodePipeline)
  # results copied to the host ride on the slot's stream: a batch queued behind one would wait for its copy, so that
  # mode keeps one batch per stream (33.8k vs 29.0k instance-timesteps/s at cfg2)
  depth = max(1, args.in_flight) if analyze else max(1, min(args.in_flight, 4))
  # small batches travel together, about 16 images to a slot and forward (DecodePipeline(coalesce=...), round 5: two batches of 8
  # +15 % at cfg2, four batches of 4 +70 % at cfg5 with the same images in flight), as long as at least two slots remain
  coalesce = 1
  if analyze and depth >= 2 and args.batch_size <= 8:
    coalesce = max(1, min(16 // max(1, args.batch_size), depth // 2))
  pipe, spans = model.pipeline(max(1, depth // coalesce), coalesce=coalesce), []
  for b0 in range(lo, hi, args.batch_size):
    b1 = min(hi, b0 + args.batch_size)
    feed = {k: v[b0:b1] for k, v in data.items() if k in ('x', 'd_in', 'y_in')}
    feed['phase_train'] = False
    if fg is not None:  # the pre-stage: the 8-bit values the pack step would store, as device tensors
      feed['y_in'], feed['d_in'] = fg.prestage(feed['x'], quantise=True)
      if cs_dir:
        sems[b0] = feed['y_in']
    left = -(-(hi - b1) // args.batch_size)  # batches still to come: the last few go out one per slot (DecodePipeline._ends_soon)
    while pipe.full(b1 - b0, remaining=left):
      consume(*(spans.pop(0) + tuple(pipe.collect())))
    pipe.submit(['y_out', 's_out'], feed, to_host=not (analyze or cs_dir), remaining=left)
    spans.append((b0, b1))
  while len(pipe):
    consume(*(spans.pop(0) + tuple(pipe.collect())))
  os.makedirs(out_dir, exist_ok=True)
  path = os.path.join(out_dir, 'pred_rank%d.npz' % rank)
  T, H, W = model.dims['T'], model.dims['H'], model.dims['W']
  # an empty shard (more ranks than images) writes empty arrays of the right rank
  y_all = np.concatenate(ys) if ys else np.zeros((0, T, H, W), np.float32)
  s_all = np.concatenate(ss) if ss else np.zeros((0, T), np.float32)
  np.savez_compressed(path, y_out=y_all, s_out=s_all, first_index=lo)
  print('rank %d: images [%d, %d) -> %s (%.2f s)' % (rank, lo, hi, path, time.time() - t0))
  if analyze:
    summary = {}
    for th in thresholds:
      vals = {n: np.concatenate(v) if v else np.zeros(0) for n, v in acc[th].items()}
      summary['%.2f' % th] = {n: {'mean': float(v.mean()) if v.size else 0.0, 'count': int(v.size)}
                              for n, v in vals.items()}
    with open(os.path.join(out_dir, 'metrics_rank%d.yaml' % rank), 'w') as f:
      yaml.safe_dump(summary, f)
    for th in sorted(summary):  # every threshold, never a ground-truth-tuned arg-max
      print('rank %d: threshold %s  %s' % (rank, th, ' '.join(
          '%s=%.4f' % (n, summary[th][n]['mean']) for n in names)))


if __name__ == '__main__':
  main()
