#!/usr/bin/env python
"""Entry point with the flag surface of the reference's fg_model_eval.py (:195-216 + EvalArgsParser): tells whether a set of
fg_model weights is any good.  For every threshold of --threshold_list (default 0.3) the foreground and background IoU over
the WHOLE data set at the labels' size (analysis.py:834-906, fg_iou_all / bg_iou_all), and, where ground truth at network size
is given, the statistics the reference's Evaluator logs while it trains the pre-stage (fg_model_train.py:131-133).

The model is restored from <results>/<model_id>/{model_opt.yaml, weights.npz} exactly as fg_model_pack.py does.  --input is an
.npz with
  x           [N,h,w,3]   the images at network size,
  fg_gt_full  [N,H,W]     uint8: the full-size labels summed over the instances (fg_model_eval.py:142-143; 2 and more where
                          instances overlap, counted as the reference's a * b and b.sum() count them),
and optionally names (N file names, default 'image_<i>') and y_gt [N,h,w] or [N,h,w,nsc] (+ d_gt [N,h,w,8] for a net with
orientation): then fg_model.Model.statistics runs on every batch and the means over the batches are reported, as the
Evaluator averages them.  The images of such an archive share one full size.  Mixed full sizes (KITTI): in place of fg_gt_full
the archive holds fg_gt_full_flat uint8 [P], pixel_offset int64 [N + 1] and orig_size int32 [N,2] (what setup_labels.py
--mixed_sizes --target fg_model writes: image i is the orig_size[i] rows from element pixel_offset[i] on).  The sweep of a batch
is then ONE ops.fg_sweep_counts_ragged call, `pixels` is summed per image, and the thresholded, soft and ground-truth PNG files
are written image by image at each image's own size through the same pp.upsample — that path writes files and is bound by the
host; run_kitti.sh feeds these PNG files to the next stage as the foreground.  --render_orientation and the pixel-level scores
(gt_instance_ids / gt_label_ids in --input) are refused by name on a mixed archive: their kernels take one size per call.

Per batch, on the device (write_log, :134-173): y_out of the net; the foreground plane is y_out[..., 0] for one semantic class
and 1 - y_out[..., 0] for several (channel 0 is the background: the convention of ops.sem_foreground — the reference's runner
only works for one class); ops.fg_sweep_counts evaluates bilateralFilter(resize(plane), 5, 10, 10) (:106-117) tile by tile,
compares it with every threshold and returns integer counters, from which analysis.ForegroundIOUAnalyzer /
BackgroundIOUAnalyzer accumulate.  The full-size soft map is materialised (pp.upsample) only for the images that are written.

Outputs: <output>/metrics.yaml — per threshold fg_iou_all, bg_iou_all and the four integer totals (count_a, sum_ab, sum_b,
pixels), plus 'statistics' when ground truth at network size was given; <output>/<NN>/<name>.png, NN = int(threshold * 100)
(:66) — the thresholded full-size map times 255 (RenderForegroundAnalyzer); <output>/soft/ and <output>/gt/ under
--render_soft / --render_gt (the soft map and the labels, times 255 and clipped to 8 bits).  --output defaults to
<results>/<model_id>/output (:184-186).  --render_ori is accepted and refused: the reference's flag renders from its HDF5
dataset's labels; the orientation image itself is built behind --render_orientation (not a reference flag): <output>/ori/<name>.png,
the colour-wheel image of data_api/orientation.py:13-28 from the model's d_out — resized to the labels' size and arg-maxed inside
one kernel (analysis.RenderOrientationAnalyzer) — with fg_gt_full > 0 as the mask; a model without add_orientation is refused.
--device_png (not a reference flag) compresses the thresholded planes, gt/ and ori/ on the device (utils/png.write_*_dev): the same
pixels in files of other bytes.  soft/ is continuous-valued, a run code would enlarge it: it stays with the host's zlib, unchanged.
On a mixed archive the thresholded planes of a batch are gathered into one flat uint8 [K,P] buffer at the geometry's offsets and
leave through ONE ragged encoder call (utils/png.write_gray8_ragged_dev: one launch chain for all thresholds and sizes), gt/
through one more on the flat labels; every file holds the bytes a call on that image alone gives.

Pixel-level class scores: when --input also holds gt_instance_ids [N,H,W] (the *_gtFine_instanceIds.png values; optionally
gt_label_ids uint8 [N,H,W], the *_gtFine_labelIds.png values, else a pixel's label is derived from its id) and the model has
nine semantic classes (the background and the eight labels of analysis.CITYSCAPES_LABELS), every batch's network-size y_out
also goes through analysis.CityscapesPixelAnalyzer in its fused form — the arg-max of the resized map is taken inside the
confusion kernel — and <output>/resultPixelLevelSemanticLabeling.json (the keys of the toolkit's
evalPixelLevelSemanticLabeling.py, plus averageScorePredictedClasses) is written beside metrics.yaml, which gains a
'pixel_level' entry with the averages.  A model with several semantic classes but not nine cannot be mapped to label ids: the
script says so and goes on without.  Without gt_instance_ids nothing changes.

No more than MAX_BATCH_ELEMS floats of one tensor are alive per batch; there is no CPU path: without a GPU the script raises
RecAttendError."""
import argparse
import os

import numpy as np
import yaml

import cmd_args_parser as cap
from ra_native import RecAttendError

MAX_BATCH_ELEMS = 1 << 29  # floats of one [B,H,W] plane at full size (2 GiB)
REFUSED = {
    'render_ori': '--render_ori renders the orientation classes as a colour image (data_api/orientation.py) from the labels of the '
                  'HDF5 dataset, which is out of scope here; --render_orientation writes that image from --input',
}
STAT_NAMES = ('iou_soft', 'iou_hard', 'foreground_loss', 'loss', 'orientation_ce', 'orientation_acc')


def build_parser():
  p = argparse.ArgumentParser(description='Eval fg output')
  cap.add_flags(p, cap.FG_EVAL_FLAGS)
  cap.add_flags(p, cap.DATA_FLAGS)
  p.add_argument('--input', default=None, help='.npz with x [N,h,w,3], fg_gt_full [N,H,W] uint8 (+ names, y_gt, d_gt)')
  p.add_argument('--render_orientation', action='store_true',
                 help='not a reference flag: write the orientation classes of the model\'s d_out as a colour-wheel image, masked '
                      'by fg_gt_full, into <output>/ori/; needs a model with add_orientation')
  cap.add_device_png_code(p)
  p.add_argument('--device_png', action='store_true',
                 help='not a reference flag: compress the thresholded planes, the --render_gt planes and the --render_orientation '
                      'images on the device (a run code within each row, utils/png.write_*_dev); the files decode to the same '
                      'pixels, their bytes differ and they are larger.  The --render_soft planes are continuous-valued, a run '
                      'code would enlarge them: they stay with the host\'s zlib and do not change')
  return p


def make_opt(args):
  """FGEvalArgsParser.make_opt (:205-216)."""
  for flag, why in REFUSED.items():
    if getattr(args, flag):
      raise RecAttendError(why)
  opt = {k: getattr(args, k) for k in ('model_id', 'batch_size', 'results', 'output', 'render_gt', 'render_soft', 'render_ori')}
  opt['split'] = args.split.split(',')
  opt['threshold_list'] = [0.3] if args.threshold_list is None else [float(t) for t in args.threshold_list.split(',')]
  return opt


def _write_planes(folder, names, planes):
  """planes: uint8 [B,H,W] on the host -> <folder>/<name>.png"""
  from utils import png
  os.makedirs(folder, exist_ok=True)
  for name, img in zip(names, planes):
    png.write_gray8(os.path.join(folder, os.path.splitext(os.path.basename(name))[0] + '.png'), img)


def _write_planes_dev(folder, names, planes, code='fixed'):
  """_write_planes for uint8 [B,H,W] planes still on the DEVICE (--device_png): one png_deflate call for the batch, in the
  stream format `code` (--device_png_code)."""
  from utils import png
  os.makedirs(folder, exist_ok=True)
  png.write_gray8_dev([os.path.join(folder, os.path.splitext(os.path.basename(name))[0] + '.png') for name in names], planes,
                      code=code)


def _write_ragged_dev(folders, names, flat, geo, code='fixed'):
  """_write_planes_dev for a batch of MIXED sizes: flat uint8 [K,P] (or [P], K = 1) on the device, every plane laid out by the
  geometry geo [B,3] -> <folders[k]>/<name>.png for every plane k and image, ONE png_deflate_ragged call."""
  from utils import png
  for folder in folders:
    os.makedirs(folder, exist_ok=True)
  png.write_gray8_ragged_dev([os.path.join(folder, os.path.splitext(os.path.basename(name))[0] + '.png') for folder in folders
                              for name in names], flat, geo, code=code)


def foreground_plane(y_out):
  """y_out [B,h,w,nsc] -> the soft foreground [B,h,w]: the only channel, or 1 - the background channel."""
  return (y_out[..., 0] if y_out.shape[-1] == 1 else 1.0 - y_out[..., 0]).contiguous()


def main(argv=None):
  import torch
  args = build_parser().parse_args(argv)
  args.device_png_code = cap.device_png_code(args)
  opt = make_opt(args)
  if args.model_id is None:
    raise Exception('You must provide model ID')  # cmd_args_parser.py:154-155
  if args.input is None:
    raise RecAttendError('--input is required: an .npz with x [N,h,w,3] and fg_gt_full [N,H,W]')
  if not torch.cuda.is_available():
    raise RecAttendError('fg_model_eval runs on the GPU; no device is available and there is no CPU fallback')
  import analysis
  import fg_model_pack
  import ra_ops as ops
  from utils import postprocess as pp
  thresholds = opt['threshold_list']
  if not 1 <= len(thresholds) <= ops.FG_SWEEP_MAX_K:
    raise RecAttendError('--threshold_list: %d thresholds (1 .. %d)' % (len(thresholds), ops.FG_SWEEP_MAX_K))
  out_dir = opt['output'] if opt['output'] is not None else os.path.join(args.results, args.model_id, 'output')
  model = fg_model_pack.restore_model(args.results, args.model_id)
  if args.render_orientation and not model.dims['no']:
    raise RecAttendError('--render_orientation: fg_model %s was built without add_orientation and has no d_out to render' % args.model_id)
  ori_render = None
  data = np.load(args.input, allow_pickle=False)
  mixed = 'fg_gt_full_flat' in data and 'fg_gt_full' not in data
  for k in ('x',) + (('fg_gt_full_flat', 'pixel_offset', 'orig_size') if mixed else ('fg_gt_full',)):
    if k not in data:
      raise RecAttendError('--input lacks %s' % k)
  if mixed:
    return _main_mixed(args, opt, data, model, out_dir, thresholds)
  x_all, gt_all = data['x'], data['fg_gt_full']
  N = x_all.shape[0]
  if gt_all.ndim != 3 or gt_all.shape[0] != N or gt_all.dtype != np.uint8:
    raise RecAttendError('--input: fg_gt_full is %s %s, expected uint8 [%d,H,W] (one full size per archive)' % (
        gt_all.dtype, tuple(gt_all.shape), N))
  H, W = gt_all.shape[1:]
  names = [str(n) for n in data['names']] if 'names' in data else ['image_%06d' % i for i in range(N)]
  have_stats = 'y_gt' in data
  y_gt_all = data['y_gt'] if have_stats else None
  d_gt_all = data['d_gt'] if have_stats and 'd_gt' in data else None
  pixel_an = None  # the toolkit's pixel-level class scores, when the archive has the instance-id images
  if 'gt_instance_ids' in data:
    nsc = int(model.opt['num_semantic_classes']) if 'num_semantic_classes' in model.opt else 1
    ids_all = data['gt_instance_ids']
    lab_all = data['gt_label_ids'] if 'gt_label_ids' in data else None
    if tuple(ids_all.shape) != (N, H, W) or not np.issubdtype(ids_all.dtype, np.integer):
      raise RecAttendError('--input: gt_instance_ids is %s %s, expected integers [%d,%d,%d]' % (ids_all.dtype, tuple(ids_all.shape), N, H, W))
    if lab_all is not None and (tuple(lab_all.shape) != (N, H, W) or lab_all.dtype != np.uint8):
      raise RecAttendError('--input: gt_label_ids is %s %s, expected uint8 [%d,%d,%d]' % (lab_all.dtype, tuple(lab_all.shape), N, H, W))
    if nsc == 1 + len(analysis.CITYSCAPES_LABELS):
      pixel_an = analysis.CityscapesPixelAnalyzer(names)
    elif nsc > 1:
      print('pixel-level class scores are left out: the model has %d semantic classes, and only %d (the background and the '
            'labels %s) map to Cityscapes label ids' % (nsc, 1 + len(analysis.CITYSCAPES_LABELS),
                                                        ', '.join(n for n, _ in analysis.CITYSCAPES_LABELS)))
  if args.render_orientation:
    ori_render = analysis.RenderOrientationAnalyzer(os.path.join(out_dir, 'ori'), [os.path.basename(n) for n in names],
                                                    device_png=args.device_png, device_png_code=args.device_png_code)
  fg_an = [analysis.ForegroundIOUAnalyzer('fg_iou_all {:.2f}'.format(t), index=k) for k, t in enumerate(thresholds)]  # :62-69
  bg_an = [analysis.BackgroundIOUAnalyzer('bg_iou_all {:.2f}'.format(t), index=k) for k, t in enumerate(thresholds)]
  totals = [{'count_a': 0, 'sum_ab': 0, 'sum_b': 0, 'pixels': 0} for _ in thresholds]
  stats = []
  os.makedirs(out_dir, exist_ok=True)
  bs = max(1, min(opt['batch_size'], MAX_BATCH_ELEMS // max(1, H * W)))
  dev = torch.device('cuda', torch.cuda.current_device())
  up = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
  to8 = lambda t: (t * 255.0).clamp(0, 255).to(torch.uint8).cpu().numpy()
  # --device_png: the same quantisation, the plane left on the device and compressed there
  write_hard = (lambda f, n, t: _write_planes_dev(f, n, (t * 255.0).clamp(0, 255).to(torch.uint8), args.device_png_code)) if args.device_png else (
      lambda f, n, t: _write_planes(f, n, to8(t)))
  for b0 in range(0, N, bs):
    b1 = min(N, b0 + bs)
    x = up(x_all[b0:b1])
    gt = torch.as_tensor(np.ascontiguousarray(gt_all[b0:b1])).to(dev)
    if ori_render is not None:
      y_out, d_out = model.run(['y_out', 'd_out'], {'x': x, 'phase_train': False})
    else:
      y_out = model.run('y_out', {'x': x, 'phase_train': False})
    soft = foreground_plane(y_out)
    if pixel_an is not None:
      res_px = {'sem': y_out.contiguous(), 'size': (H, W), 'indices': list(range(b0, b1)),
                'gt_ids': torch.as_tensor(np.ascontiguousarray(ids_all[b0:b1].astype(np.int32, copy=False))).to(dev)}
      if lab_all is not None:
        res_px['gt_labels'] = torch.as_tensor(np.ascontiguousarray(lab_all[b0:b1])).to(dev)
      pixel_an.stage(res_px)
    counts = ops.fg_sweep_counts(soft, gt, thresholds)
    res = {'fg_counts': counts, 'indices': list(range(b0, b1))}
    for k in range(len(thresholds)):
      fg_an[k].stage(res)
      bg_an[k].stage(res)
      totals[k]['count_a'] += int(counts['count_a'][:, k].sum())
      totals[k]['sum_ab'] += int(counts['sum_ab'][:, k].sum())
      totals[k]['sum_b'] += int(counts['sum_b'].sum())
      totals[k]['pixels'] += counts['pixels'] * (b1 - b0)
    full = pp.upsample(soft, (H, W))  # the rendering path only: :146, :166-173
    for t in thresholds:
      write_hard(os.path.join(out_dir, '{:02d}'.format(int(t * 100))), names[b0:b1], (full > float(t)).to(torch.float32))
    if opt['render_soft']:
      _write_planes(os.path.join(out_dir, 'soft'), names[b0:b1], to8(full))
    if opt['render_gt']:
      write_hard(os.path.join(out_dir, 'gt'), names[b0:b1], gt.to(torch.float32))
    if ori_render is not None:  # :154-164: d_out at network size, the labels as the mask
      ori_render.stage({'d_out': d_out.contiguous(), 'mask': (gt > 0).to(torch.float32), 'indices': list(range(b0, b1))})
    if have_stats:
      stats.append(model.statistics(x, up(y_gt_all[b0:b1]), None if d_gt_all is None else up(d_gt_all[b0:b1])))
  summary = {}
  for k, t in enumerate(thresholds):
    summary['%.2f' % t] = dict(totals[k], fg_iou_all=float(fg_an[k].finalize()), bg_iou_all=float(bg_an[k].finalize()))
  if have_stats:
    summary['statistics'] = {n: float(np.mean([s[n] for s in stats])) for n in STAT_NAMES if n in stats[0]}
    for n, v in summary['statistics'].items():
      print('{:17s}{:7.4f}'.format(n, v))
  if pixel_an is not None:
    px = pixel_an.finalize(os.path.join(out_dir, 'resultPixelLevelSemanticLabeling.json'))
    summary['pixel_level'] = {k: float(px[k]) for k in sorted(px) if k.startswith('averageScore')}
  with open(os.path.join(out_dir, 'metrics.yaml'), 'w') as f:
    yaml.safe_dump(summary, f)
  print('%d images -> %s' % (N, out_dir))
  return summary


def _main_mixed(args, opt, data, model, out_dir, thresholds):
  """main() on an archive of mixed full sizes: fg_gt_full_flat, pixel_offset, orig_size (the module's docstring)."""
  import torch
  import analysis
  import ra_ops as ops
  import setup_labels
  from utils import postprocess as pp
  if args.render_orientation:
    raise RecAttendError('--render_orientation cannot be used with an --input of mixed full sizes (%s holds fg_gt_full_flat): the '
                         'orientation image is rendered for one full size per call' % args.input)
  for k in ('gt_instance_ids', 'gt_label_ids'):
    if k in data:
      raise RecAttendError('the pixel-level class scores (%s in --input) cannot be computed on an --input of mixed full sizes (%s '
                           'holds fg_gt_full_flat): the confusion kernels take one full size per call' % (k, args.input))
  x_all, gt_all, off, size = data['x'], data['fg_gt_full_flat'], data['pixel_offset'], data['orig_size']
  N = x_all.shape[0]
  if gt_all.dtype != np.uint8:
    raise RecAttendError('--input: fg_gt_full_flat is %s, expected uint8 [P]' % gt_all.dtype)
  setup_labels.check_flat('--input %s' % args.input, gt_all, off, size, N)
  names = [str(n) for n in data['names']] if 'names' in data else ['image_%06d' % i for i in range(N)]
  if len(names) != N:
    raise RecAttendError('--input: %d names for %d images' % (len(names), N))
  have_stats = 'y_gt' in data
  y_gt_all = data['y_gt'] if have_stats else None
  d_gt_all = data['d_gt'] if have_stats and 'd_gt' in data else None
  fg_an = [analysis.ForegroundIOUAnalyzer('fg_iou_all {:.2f}'.format(t), index=k) for k, t in enumerate(thresholds)]  # :62-69
  bg_an = [analysis.BackgroundIOUAnalyzer('bg_iou_all {:.2f}'.format(t), index=k) for k, t in enumerate(thresholds)]
  totals = [{'count_a': 0, 'sum_ab': 0, 'sum_b': 0, 'pixels': 0} for _ in thresholds]
  stats = []
  os.makedirs(out_dir, exist_ok=True)
  dev = torch.device('cuda', torch.cuda.current_device())
  up = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
  quant = lambda t: (t * 255.0).clamp(0, 255).to(torch.uint8)  # --device_png: the same quantisation, left on the device
  to8 = lambda t: quant(t).cpu().numpy()
  write_hard = lambda f, n, t: _write_planes(f, n, to8(t))
  bs = max(1, opt['batch_size'])
  for b0 in range(0, N, bs):
    b1 = min(N, b0 + bs)
    p0, p1 = int(off[b0]), int(off[b1])
    geo = setup_labels.flat_geometry(off, size, b0, b1)
    x = up(x_all[b0:b1])
    gt = torch.as_tensor(np.ascontiguousarray(gt_all[p0:p1])).to(dev)
    soft = foreground_plane(model.run('y_out', {'x': x, 'phase_train': False}))
    counts = ops.fg_sweep_counts_ragged(soft, gt, geo, thresholds)  # one launch chain for the batch, whatever its sizes
    res = {'fg_counts': counts, 'indices': list(range(b0, b1))}
    for k in range(len(thresholds)):
      fg_an[k].stage(res)
      bg_an[k].stage(res)
      totals[k]['count_a'] += int(counts['count_a'][:, k].sum())
      totals[k]['sum_ab'] += int(counts['sum_ab'][:, k].sum())
      totals[k]['sum_b'] += int(counts['sum_b'].sum())
      totals[k]['pixels'] += int(counts['pixels'].sum())
    # --device_png: the thresholded planes of the whole batch in ONE flat uint8 [K,P_batch] buffer, image i at the geometry's
    # offset, encoded by one ragged call (one launch chain, whatever the sizes); gt/ is one more call on the flat gt
    hard = torch.zeros((len(thresholds), p1 - p0), dtype=torch.uint8, device=dev) if args.device_png else None
    for i, (o, h, w) in enumerate(geo.tolist()):  # the rendering path only (:146, :166-173), image by image at its own size
      full = pp.upsample(soft[i:i + 1].contiguous(), (h, w))
      for k, t in enumerate(thresholds):
        if hard is not None:
          hard[k, o:o + h * w] = quant((full > float(t)).to(torch.float32)).view(-1)
        else:
          write_hard(os.path.join(out_dir, '{:02d}'.format(int(t * 100))), names[b0 + i:b0 + i + 1], (full > float(t)).to(torch.float32))
      if opt['render_soft']:
        _write_planes(os.path.join(out_dir, 'soft'), names[b0 + i:b0 + i + 1], to8(full))
      if opt['render_gt'] and hard is None:
        write_hard(os.path.join(out_dir, 'gt'), names[b0 + i:b0 + i + 1], gt[o:o + h * w].view(1, h, w).to(torch.float32))
    if hard is not None:
      _write_ragged_dev([os.path.join(out_dir, '{:02d}'.format(int(t * 100))) for t in thresholds], names[b0:b1], hard, geo,
                        args.device_png_code)
      if opt['render_gt']:
        _write_ragged_dev([os.path.join(out_dir, 'gt')], names[b0:b1], quant(gt.to(torch.float32)), geo, args.device_png_code)
    if have_stats:
      stats.append(model.statistics(x, up(y_gt_all[b0:b1]), None if d_gt_all is None else up(d_gt_all[b0:b1])))
  summary = {}
  for k, t in enumerate(thresholds):
    summary['%.2f' % t] = dict(totals[k], fg_iou_all=float(fg_an[k].finalize()), bg_iou_all=float(bg_an[k].finalize()))
  if have_stats:
    summary['statistics'] = {n: float(np.mean([s[n] for s in stats])) for n in STAT_NAMES if n in stats[0]}
    for n, v in summary['statistics'].items():
      print('{:17s}{:7.4f}'.format(n, v))
  with open(os.path.join(out_dir, 'metrics.yaml'), 'w') as f:
    yaml.safe_dump(summary, f)
  print('%d images of mixed sizes -> %s' % (N, out_dir))
  return summary


if __name__ == '__main__':
  main()
