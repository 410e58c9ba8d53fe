"""analysis.py of the reference (the metric functions, :314-787) on the MI355X.

`results` is the dict full_model_eval.py:128-135 builds — 'y_out' (thresholded, [B,T,H,W]),
'y_gt', 's_out', 's_gt' — with float32 CUDA tensors.  All functions share one device pass
(ops.eval_metrics: pairwise intersections on the MFMA streaming kernel + one small metrics
kernel), cached on the dict as results['_metrics'].  A caller that has the numbers already puts them there itself and needs
no masks at all: full_model_eval.py's id-image path hands over ops.eval_metrics_from_counts' dict (the same metrics kernel, fed
the integers of ops.instance_eval_counts), with 's_out' and 's_gt' beside it.  Of the analyzers that render images or write CSV files (:52-311, :790-900) these are built:
CountAnalyzer (:67-92), RenderInstanceAnalyzer (:95-153), RenderGroundtruthInstanceAnalyzer (:156-193) and
RenderOrientationAnalyzer (:270-283) — the colour images are composed on the device (ops.render_instances /
ops.render_orientation) and written by utils/png.py — and RenderCityScapesOutputAnalyzer (:196-267, the Cityscapes
instance-level output).  StatsAnalyzer's per-metric CSV files (:790-831), RenderForegroundAnalyzer (fg_model_eval.py writes
those planes itself) and the plots stay out of scope.  ForegroundIOUAnalyzer / BackgroundIOUAnalyzer
(:834-906) accumulate over a whole dataset, in
exact integers, from the counters of ops.fg_sweep_counts; fg_model_eval.py drives them and they are not per-image functions,
so ANALYZERS does not list them."""
import os

import torch

import ra_ops as ops


def _m(results):
  if '_metrics' not in results:
    results['_metrics'] = ops.eval_metrics(results['y_out'], results['y_gt'], results['s_gt'])
    if 'iou_pairwise' not in results:
      results['iou_pairwise'] = results['_metrics']['iou_pairwise']
  return results['_metrics']


def _stat(results, name):
  return _m(results)['stats'][:, ops.EVAL_NAMES.index(name)]


def _inst(results, name):
  return _m(results)['inst'][:, ops.EVALI_NAMES.index(name)]


def f_iou_pairwise(a, b):
  """:329-334 for batches: a [B,N,H,W], b [B,M,H,W] binary -> [B,N,M]."""
  st = ops.pair_stats(a, b, want=('inter', 'sum_a', 'sum_b'))
  union = st['sum_a'][:, :, None] + st['sum_b'][:, None, :] - st['inter']
  return st['inter'] / (union + (union == 0).to(torch.float32))


def f_iou(a, b):
  """:314-326 for aligned [B,N,H,W] masks -> [B,N]."""
  return torch.diagonal(f_iou_pairwise(a, b), dim1=1, dim2=2)


def f_symmetric_best_dice(results):
  """:434-460 -> [B]."""
  return _stat(results, 'sbd')


def f_coverage(results, weighted=False):
  """:481-504."""
  return _stat(results, 'wt_cov' if weighted else 'unwt_cov')


def f_wt_coverage(results):
  return f_coverage(results, weighted=True)


def f_unwt_coverage(results):
  return f_coverage(results, weighted=False)


def f_fg_iou(results):
  """:533-553."""
  return _stat(results, 'fg_iou')


def f_fg_dice(results):
  """:556-576."""
  return _stat(results, 'fg_dice')


def f_fp(results):
  """:579-592."""
  return _stat(results, 'avg_fp')


def f_fn(results):
  """:595-605."""
  return _stat(results, 'avg_fn')


def f_pixel_pr(results):
  """:608-627 -> 1-D tensor over the output instances that exist."""
  return _inst(results, 'pix_pr')[_inst(results, 'has_out') > 0]


def f_pixel_re(results):
  """:630-650 -> 1-D tensor over the ground-truth instances."""
  return _inst(results, 'pix_re')[_inst(results, 'is_gt') > 0]


def f_obj_pr(results):
  """:653-671."""
  return _inst(results, 'obj_pr')[_inst(results, 'has_out') > 0]


def f_obj_re(results):
  """:674-690."""
  return _inst(results, 'obj_re')[_inst(results, 'is_gt') > 0]


def f_count_mse(results):
  """:693-708."""
  return _stat(results, 'count_mse')


def f_count_acc(results):
  """:711-726."""
  return _stat(results, 'count_acc')


def f_dic(results):
  """:729-744."""
  return _stat(results, 'dic')


def f_dic_abs(results):
  """:747-763."""
  return _stat(results, 'dic_abs')


def f_count_out(y_out):
  """:766-770."""
  sizes = ops.pair_stats(y_out, y_out[:, :1], want=('sum_a',))['sum_a']
  return (sizes > 0).to(torch.float32)


ANALYZERS = {'sbd': f_symmetric_best_dice, 'wt_cov': f_wt_coverage, 'unwt_cov': f_unwt_coverage,
             'fg_dice': f_fg_dice, 'fg_iou': f_fg_iou, 'avg_fp': f_fp, 'avg_fn': f_fn,
             'avg_pr': f_pixel_pr, 'avg_re': f_pixel_re, 'obj_pr': f_obj_pr, 'obj_re': f_obj_re,
             'count_acc': f_count_acc, 'count_mse': f_count_mse, 'dic': f_dic, 'dic_abs': f_dic_abs}


def create_analyzer(name, display_name=None, fname=None):
  """:9-49 reduced to the metric function: returns f(results) -> tensor; the StatsAnalyzer
  wrapper that accumulates and writes CSV (:790-831) is out of scope."""
  name = name.lower()
  if name not in ANALYZERS:
    raise Exception('Analyzer not found: {}'.format(name))
  return ANALYZERS[name]


def f_ins_iou(results):
  raise NotImplementedError('f_ins_iou (:404-431) indexes the whole-batch list instead of one example '
                            '(iou_pairwise vs iou_pairwise_) and cannot run in the reference either')


# ---- the Cityscapes instance-level output (:196-267) ----
CITYSCAPES_LABELS = [('person', 24), ('rider', 25), ('car', 26), ('truck', 27), ('bus', 28), ('train', 31),
                     ('motorcycle', 32), ('bicycle', 33)]  # :203-210


def f_instance_class(results):
  """:232-261 without the files.  results: 'y_out' [B,T,H,W] (the thresholded masks at the labels' size), 'y_in' the
  semantic map at NETWORK size [B,Hs,Ws,C] (the reference hands over the resized map; here the resize is evaluated inside
  the vote kernel), 'conf' [B,T].  Returns (class_idx, label_id, vote): int32 [B,T] (-1 = not written), int32 [B,T] (the
  Cityscapes id from CITYSCAPES_LABELS, -1 = not written), float32 [B,T,C].  An instance is written when conf > 0.5 and
  vote[0] <= 0.7; vote[0] is a mean over the whole image, so that gate almost never closes — the reference's rule."""
  if '_instance_class' not in results:
    vote, idx, lab = ops.instance_class_vote(results['y_out'], results['y_in'], results['conf'])
    results['_instance_class'] = (idx, lab, vote)
  return results['_instance_class']


def _stem(name):
  # the reference writes fn1.strip('.png'), which also eats leading / trailing 'p', 'n', 'g' and '.' characters of the
  # name itself; here only the extension goes
  return name[:-4] if name.endswith('.png') else name


def cityscapes_line(img_file, label_id, score):
  """:258-259."""
  return '{} {:d} {:f}\n'.format(img_file, int(label_id), float(score))


def _png_code(code):
  """device_png_code of the analyzers that write PNG files: the device encoder's stream format."""
  if code not in ('fixed', 'dynamic'):
    raise ValueError("device_png_code=%r (one of 'fixed', 'dynamic')" % (code,))
  return code


class RenderCityScapesOutputAnalyzer(object):
  """:196-267.  names: the file name of every image ('<run>_<seq>_<frame>...[.png]', what dataset.get_fname returns there),
  indexed by results['indices'].  stage() writes <folder>/<run>/<name>.txt — one line '<name>_<t:03d>.png <label_id> <score>'
  per written instance — and every written mask as an 8-bit PNG, (seg * 255).astype('uint8'); <run> is the name up to its
  first '_'.  As in the reference the text file is opened anew by every stage() call: with several thresholds sharing one
  folder the last one staged is what remains.  device_png: the masks are compressed on the device (utils/png.write_gray8_dev:
  ONE ops.png_deflate call per stage() over the kept (ii, jj) planes of y_out, read as floats and never materialised as uint8)
  instead of copied to the host plane by plane; the files decode to the same pixels, their bytes differ.  device_png_code:
  the device encoder's stream format, 'fixed' or 'dynamic' (one dynamic-Huffman block per image: about a fifth of the bytes)."""

  def __init__(self, folder, names, device_png=False, device_png_code='fixed'):
    if folder is None:
      raise Exception('No output folder')
    self.folder = folder
    self.names = list(names)
    self.device_png = bool(device_png)
    self.device_png_code = _png_code(device_png_code)
    self.labels = CITYSCAPES_LABELS
    self.written = []  # (text file, [(png file, label_id, score), ...]) per staged image
    os.makedirs(folder, exist_ok=True)

  def stage(self, results):
    from utils import png
    idx, lab, _ = f_instance_class(results)
    y_out, indices = results['y_out'], results['indices']
    idx_h, lab_h = idx.cpu().numpy(), lab.cpu().numpy()
    if ((idx_h >= 0) & (lab_h < 0)).any():  # the reference's self.labels[sem_idx] raises there too
      raise IndexError('a class index beyond the %d Cityscapes instance classes' % len(self.labels))
    score = results['conf'].cpu().numpy()
    kept = []  # device_png: (plane of y_out as [B * T, H, W], path) of every mask to write
    for ii in range(y_out.shape[0]):
      fn1 = _stem(str(self.names[int(indices[ii])]))
      runfolder = os.path.join(self.folder, fn1.split('_')[0])
      os.makedirs(runfolder, exist_ok=True)
      text_fn = os.path.join(runfolder, fn1 + '.txt')
      lines = []
      with open(text_fn, 'w') as text_file:
        for jj in range(y_out.shape[1]):
          if idx_h[ii, jj] < 0:
            continue
          img_file = fn1 + '_{:03d}.png'.format(jj)
          if self.device_png:
            kept.append((ii * y_out.shape[1] + jj, os.path.join(runfolder, img_file)))
          else:
            seg = (y_out[ii, jj] * 255).to(torch.uint8).cpu().numpy()
            png.write_gray8(os.path.join(runfolder, img_file), seg)
          text_file.write(cityscapes_line(img_file, lab_h[ii, jj], score[ii, jj]))
          lines.append((img_file, int(lab_h[ii, jj]), float(score[ii, jj])))
      self.written.append((text_fn, lines))
    if kept:
      planes = y_out.contiguous().to(torch.float32).view(-1, y_out.shape[2], y_out.shape[3])
      png.write_gray8_dev([path for _, path in kept], planes, [k for k, _ in kept], code=self.device_png_code)

  def finalize(self):
    pass


# ---- the colour images and the count file (:67-193, :270-283) ----
# :103-124, one row per instance slot (row t % 22).  The reference's last row reads [319, 29, 82] in a uint8 array, which
# old NumPy stores as 319 mod 256 = 63 (NumPy 2 raises on it): 63 is what it draws with.
# Channel convention: the instance analyzers swap [2, 1, 0] before cv2.imwrite (:147, :187), so a row is the R, G, B of the FILE.
INSTANCE_CMAP = ((192, 57, 43), (243, 156, 18), (26, 188, 156), (41, 128, 185), (142, 68, 173), (44, 62, 80), (127, 140, 141),
                 (17, 75, 95), (2, 128, 144), (228, 253, 225), (69, 105, 144), (244, 91, 105), (91, 192, 235), (253, 231, 76),
                 (155, 197, 61), (229, 89, 52), (250, 121, 33), (124, 82, 47), (86, 15, 94), (38, 63, 77), (1, 52, 55),
                 (63, 29, 82))
# data_api/orientation.py:3-11, one row per orientation class.  Channel convention: build_orientation_img's array goes to
# cv2.imwrite UNSWAPPED (:278-282), so a row is the B, G, R of the file — the file's R, G, B is the row REVERSED.
ORIENTATION_WHEEL = ((255, 17, 0), (255, 137, 0), (230, 255, 0), (34, 255, 0), (0, 255, 213), (0, 154, 255), (9, 0, 255),
                     (255, 0, 255))


def groundtruth_colours(iou_pairwise):
  """:168-182 on the host: the colour of every ground-truth plane from iou_pairwise [B,T_out,T_gt] (what _m caches) -> uint8
  [B,T_gt,3], rows of INSTANCE_CMAP (the file's R, G, B).  Per image, in the order of the planes: the output with the largest
  IoU (first maximum; an empty plane's column is all zero, so 0) names the colour; if that colour is taken, the first free
  one counted from the END of the palette; with all 22 taken the previous plane's colour stays.  Every plane consumes a colour,
  empty ones too.  A winning index >= 22 raises IndexError, as the reference's flag[max_idx] does."""
  import numpy as np
  iou = iou_pairwise.detach().cpu().numpy() if isinstance(iou_pairwise, torch.Tensor) else np.asarray(iou_pairwise)
  if iou.ndim != 3 or iou.shape[1] < 1:
    raise ValueError('groundtruth_colours: iou_pairwise must be [B,T_out,T_gt] with T_out >= 1, got %s' % (iou.shape,))
  cmap = np.array(INSTANCE_CMAP, dtype=np.uint8)
  n = cmap.shape[0]
  out = np.zeros((iou.shape[0], iou.shape[2], 3), dtype=np.uint8)
  for ii in range(iou.shape[0]):
    used = [False] * n
    colour = None
    for jj in range(iou.shape[2]):
      best = int(np.argmax(iou[ii, :, jj]))
      if best >= n:
        raise IndexError('index %d is out of bounds for the %d colours of the palette' % (best, n))
      if not used[best]:
        colour, used[best] = cmap[best], True
      else:
        for idx in range(n - 1, -1, -1):
          if not used[idx]:
            colour, used[idx] = cmap[idx], True
            break
      out[ii, jj] = colour
  return out


class CountAnalyzer(object):
  """:67-92.  The file starts with the header line; stage() appends '<index>,<count out>,<count gt>' per image, from
  f_count_out(y_out).sum(1) (the output planes that have a pixel) and s_gt.sum(1).  Results of the id path hold no y_out: there
  the planes that have a pixel are the non-zero entries of results['_metrics']['sizes'] [B,T], the counted areas."""

  def __init__(self, fname):
    self.fname = fname
    with open(fname, 'w') as f:
      f.write('Image ID,Count Out,Count GT\n')  # :72

  def stage(self, results):
    if 'y_out' not in results and 'sizes' in results.get('_metrics', {}):
      count_out = (results['_metrics']['sizes'] > 0).sum(dim=1).cpu().numpy()
    else:
      count_out = f_count_out(results['y_out']).sum(dim=1).cpu().numpy()
    count_gt = results['s_gt'].sum(dim=1).cpu().numpy()
    with open(self.fname, 'a') as f:
      for ii, idx in enumerate(results['indices']):
        f.write('{},{:d},{:d}\n'.format(idx, int(count_out[ii]), int(count_gt[ii])))  # :85-86

  def finalize(self):
    pass


class RaggedPicture(object):
  """One picture per image of a batch of MIXED sizes as it lies on the device: flat uint8 [P,3] (one plane of what
  ops.paint_instances(..., geo=...) or ops.paint_groundtruth(..., geo=...) writes) and its geometry [B,3] of (offset, h, w).
  It has len(), iterates and indexes as the list of [h,w,3] views into `flat` that it replaces, so whoever takes such a list
  takes this; the render analyzers' device_png route reads .flat and .geo and encodes the batch in one call."""

  def __init__(self, flat, geo):
    import numpy as np
    geo = np.asarray(geo)
    if flat.dim() != 2 or flat.shape[1] != 3 or geo.ndim != 2 or geo.shape[1] != 3:
      raise ops.rn.RecAttendError('RaggedPicture: flat must be [P,3] and geo [B,3] of (offset, h, w), got %s and %s' % (
          tuple(flat.shape), geo.shape))
    self.flat, self.geo = flat, geo

  def __len__(self):
    return int(self.geo.shape[0])

  def __getitem__(self, ii):
    if isinstance(ii, slice):
      return [self[k] for k in range(*ii.indices(len(self)))]
    o, h, w = (int(v) for v in self.geo[ii])
    return self.flat[o:o + h * w].view(h, w, 3)

  def __iter__(self):
    return (self[ii] for ii in range(len(self)))


class _RenderBase(object):
  """names: the file name of every image, indexed by results['indices']; an image goes to <folder>/<name without .png>.png.
  device_png: the batch is compressed on the device (utils/png.write_colour8_dev, one ops.png_deflate call; a batch of mixed
  sizes: write_colour8_ragged_dev, one ops.png_deflate_ragged call) and only the streams are copied; the files decode to the
  same pixels, their bytes differ.  device_png_code: the device encoder's stream format, 'fixed' or 'dynamic'."""

  def __init__(self, folder, names, device_png=False, device_png_code='fixed'):
    if folder is None:
      raise Exception('No output folder')
    self.folder = folder
    self.names = list(names)
    self.device_png = bool(device_png)
    self.device_png_code = _png_code(device_png_code)
    self.written = []
    os.makedirs(folder, exist_ok=True)

  def _write(self, img, indices):
    from utils import png
    if self.device_png:
      paths = [os.path.join(self.folder, _stem(str(self.names[int(indices[ii])])) + '.png') for ii in range(img.shape[0])]
      self.written += png.write_colour8_dev(paths, img, code=self.device_png_code)
      return
    host = img.cpu().numpy()
    for ii in range(host.shape[0]):
      path = os.path.join(self.folder, _stem(str(self.names[int(indices[ii])])) + '.png')
      png.write_colour8(path, host[ii])
      self.written.append(path)

  def _write_pictures(self, picture, indices):
    """results['picture'] of the id path, painted already (ops.paint_instances / ops.paint_groundtruth): a uint8 [B,H,W,3]
    batch, or — a batch of mixed sizes — a RaggedPicture or a list of [h,w,3] views.  With device_png a RaggedPicture is
    encoded where it lies, ONE write_colour8_ragged_dev call (one launch chain) for the batch whatever the mix of sizes; the
    images of a plain list are encoded one write_colour8_dev call per group of equal size."""
    if not isinstance(picture, (list, tuple, RaggedPicture)):
      return self._write(picture, indices)
    if len(picture) != len(indices):
      raise ops.rn.RecAttendError('%s: %d pictures for %d indices' % (type(self).__name__, len(picture), len(indices)))
    if self.device_png and isinstance(picture, RaggedPicture):
      from utils import png
      paths = [os.path.join(self.folder, _stem(str(self.names[int(ii)])) + '.png') for ii in indices]
      self.written += png.write_colour8_ragged_dev(paths, picture.flat, picture.geo, code=self.device_png_code)
      return
    groups = {}
    for ii, p in enumerate(picture):
      groups.setdefault(tuple(p.shape) if self.device_png else ii, []).append(ii)
    for members in groups.values():
      self._write(torch.stack([picture[ii] for ii in members]), [indices[ii] for ii in members])

  def finalize(self):
    pass


class RenderInstanceAnalyzer(_RenderBase):
  """:95-153: one colour image per input, every plane of results['y_out'] [B,T,H,W] in its own colour (INSTANCE_CMAP[t % 22]),
  summed in uint8 as the reference sums them (overlaps wrap).  One launch of ops.render_instances; the file's R, G, B is
  the cmap row (the reference swaps before cv2.imwrite).  Results that carry 'picture' in place of 'y_out' (the id path) are
  written as they are."""

  def stage(self, results):
    if 'picture' in results:
      return self._write_pictures(results['picture'], results['indices'])
    self._write(ops.render_instances(results['y_out']), results['indices'])


class RenderGroundtruthInstanceAnalyzer(_RenderBase):
  """:156-193: the ground truth results['y_gt'] [B,T_gt,H,W], every plane in the colour of its best-matching prediction
  (groundtruth_colours on results['iou_pairwise'], chosen on the host), an earlier plane on top — per channel, as there.  One
  RA_RENDER_FIRST launch.  'iou_pairwise' is what the metrics pass (_m) caches on the dict; where no metric has run it is
  f_iou_pairwise(y_out, y_gt), which takes any pair of plane counts, and is cached likewise."""

  def stage(self, results):
    import numpy as np
    if 'picture' in results:  # the id path: painted from the id image with groundtruth_colours of the same iou_pairwise
      return self._write_pictures(results['picture'], results['indices'])
    if 'iou_pairwise' not in results:
      results['iou_pairwise'] = f_iou_pairwise(results['y_out'], results['y_gt'])
    y_gt = results['y_gt']
    rgb = groundtruth_colours(results['iou_pairwise'])
    if rgb.shape[:2] != tuple(y_gt.shape[:2]):
      raise ops.rn.RecAttendError('RenderGroundtruthInstanceAnalyzer: iou_pairwise gives colours for %s planes, y_gt is %s' % (
          rgb.shape[:2], tuple(y_gt.shape)))
    bgr = torch.as_tensor(np.ascontiguousarray(rgb[:, :, ::-1])).to(y_gt.device)  # the image's memory order
    self._write(ops.render_instances(y_gt, colours=bgr, first=True), results['indices'])


class RenderOrientationAnalyzer(_RenderBase):
  """:270-283 with fg_model_eval.py:128-132,154-164: results['d_out'] [B,Hs,Ws,C] at NETWORK size (the reference hands over
  the resized planes; here the resize is evaluated inside the kernel) and results['mask'] [B,H,W] of 0 / 1 at full size ->
  the wheel colour of the arg-max class times the mask.  The array goes to the file unswapped there, so the file's R, G, B
  is the ORIENTATION_WHEEL row reversed."""

  def stage(self, results):
    self._write(ops.render_orientation(results['d_out'], results['mask']), results['indices'])


# ---- Cityscapes instance-level AP(data_api/cityscapes_scripts/evaluation/evalInstanceLevelSemanticLabeling.py) ----
# Line numbers below are that script's.  The pixel work (assignGt2Preds' count_nonzero per prediction and ground-truth
# instance, :306-333) runs on the device (ops.gt_instance_catalog, ops.instance_overlap); what is left is a few hundred
# integers per image, the MATCH RECORD, and float64 NumPy on those.
AP_MIN_REGION_SIZES = [100, 1000, 1000]            # :136; only the first is used without distances (:386-389)
AP_DISTANCE_THS = [float('inf'), 100.0, 50.0]      # :138
AP_DISTANCE_CONFS = [-float('inf'), 0.5, 0.5]      # :140
# label ids with ignoreInEval in helpers/labels.py (:282-286); its id -1 (license plate) cannot occur in a 16-bit image
AP_VOID_LABEL_IDS = (0, 1, 2, 3, 4, 5, 6, 9, 10, 14, 15, 16, 18, 29, 30)


def _ap_overlaps():
  import numpy as np
  return np.arange(0.5, 1., 0.05)


def cityscapes_match_record(gt_ids, gt_pixels, inter, pred_pixels, label_id, conf):
  """The match record of one image (assignGt2Preds, :260-353) from host arrays: gt_ids, gt_pixels [G] the image's catalogue
  (distinct raw values of the instance-id image, ascending, and their pixel counts), inter [T,G] and pred_pixels [T] the
  overlap counts, label_id [T] (-1 = not written), conf [T].  A prediction is kept when its label is one of the eight
  evaluated classes and it has pixels (:297-311); its confidence is what the script would read back from the text file,
  float('%f' % conf); its void intersection is the sum of inter over entries whose RAW value is an ignoreInEval label id
  (:282-286,:321).  Returns a dict of arrays: gt_id, gt_pixels [G]; pred_label, pred_pixels, pred_void [P] int64, pred_conf
  [P] float64, inter [P,G] int64."""
  import numpy as np
  gt_ids = np.asarray(gt_ids, np.int64).reshape(-1)
  gt_pixels = np.asarray(gt_pixels, np.int64).reshape(-1)
  inter = np.asarray(inter, np.int64).reshape(-1, gt_ids.size)
  pred_pixels = np.asarray(pred_pixels, np.int64).reshape(-1)
  label_id = np.asarray(label_id, np.int64).reshape(-1)
  conf = np.asarray(conf, np.float64).reshape(-1)
  evaluated = [l for _, l in CITYSCAPES_LABELS]
  keep = np.array([int(l) in evaluated and int(n) > 0 for l, n in zip(label_id, pred_pixels)], bool)
  void = np.isin(gt_ids, AP_VOID_LABEL_IDS)
  return {'gt_id': gt_ids, 'gt_pixels': gt_pixels, 'pred_label': label_id[keep], 'pred_pixels': pred_pixels[keep],
          'pred_void': inter[keep][:, void].sum(axis=1), 'pred_conf': np.array([float('%f' % c) for c in conf[keep]], np.float64),
          'inter': inter[keep]}


def _ap_of_curve(y_true, y_score, hard_fns):
  """:490-543: the area under the precision-recall curve of the examples (y_true 0 / 1, y_score), one point per distinct
  score plus the point (recall 0, precision 1), integrated with steps of half the recall difference of the neighbours."""
  import numpy as np
  order = np.argsort(y_score, kind='stable')
  score, true = y_score[order], y_true[order]
  below_incl = np.cumsum(true)
  _, first = np.unique(score, return_index=True)
  n_true = below_incl[-1]
  below = np.where(first > 0, below_incl[first - 1], 0.0)  # true examples scored below each threshold
  tp = n_true - below
  fp = (score.size - first) - tp
  fn = below + hard_fns
  precision = np.append(tp / (tp + fp), 1.0)
  recall = np.append(tp / (tp + fn), 0.0)
  ext = np.concatenate([recall[:1], recall, [0.0]])
  return float(np.dot(precision, 0.5 * (ext[:-2] - ext[2:])))


def cityscapes_ap(records, min_region=AP_MIN_REGION_SIZES[0]):
  """evaluateMatches (:356-551) without distance terms (distanceAvailable = False) on a list of match records -> ap
  [1, 8 classes, 10 overlaps] float64.  Per class and overlap threshold, per image: a ground-truth instance (raw id >= 1000,
  at least min_region pixels) is matched by every prediction of its class with IoU above the threshold; the best-scored one
  makes it a true example and every other one a false positive (:438-445); an instance without a match is a hard false
  negative.  A prediction that matches no ground-truth entry of its class at all (groups and small instances included) is
  a false positive unless more than the threshold of its pixels lie on void, on a group (raw id < 1000) or on an instance
  below min_region (:468-483).  A class with no ground truth and no prediction gives NaN, with ground truth only 0.  Should
  every prediction of a class be ignored and no instance be matched there are no examples at all; the script fails on that
  (an index into an empty cumulative sum), here the AP is 0."""
  import numpy as np
  overlaps = _ap_overlaps()
  ap = np.zeros((1, len(CITYSCAPES_LABELS), len(overlaps)), np.float64)
  for li, (_, label) in enumerate(CITYSCAPES_LABELS):
    per_image = []
    have_gt = have_pred = False
    for r in records:
      gid = r['gt_id']
      cols = np.where(np.where(gid < 1000, gid, gid // 1000) == label)[0]
      rows = np.where(r['pred_label'] == label)[0]
      gpix = r['gt_pixels'][cols].astype(np.float64)
      ppix = r['pred_pixels'][rows].astype(np.float64)
      inter = r['inter'][np.ix_(rows, cols)].astype(np.float64)
      iou = inter / (gpix[None, :] + ppix[:, None] - inter) if inter.size else inter  # > 0 wherever the union is
      real = (gid[cols] >= 1000) & (r['gt_pixels'][cols] >= min_region)
      ignore = r['pred_void'][rows].astype(np.float64) + (inter * ((gid[cols] < 1000).astype(np.float64) +
                                                                   (r['gt_pixels'][cols] < min_region))[None, :]).sum(axis=1)
      have_gt |= bool(real.any())
      have_pred |= rows.size > 0
      per_image.append((inter > 0, iou, real, ignore / np.maximum(ppix, 1.0), r['pred_conf'][rows]))
    for oi, th in enumerate(overlaps):
      if not (have_gt and have_pred):
        ap[0, li, oi] = 0.0 if have_gt else float('nan')
        continue
      trues, scores, hard_fns = [], [], 0
      for touch, iou, real, ignored, conf in per_image:
        hit = touch & (iou > th)
        for g in np.where(real)[0]:
          c = np.sort(conf[hit[:, g]])
          if c.size == 0:
            hard_fns += 1
            continue
          trues += [1.0] + [0.0] * (c.size - 1)  # the best score is the match, the others are false positives
          scores += [c[-1]] + c[:-1].tolist()
        lone = ~hit.any(axis=1) & (ignored <= th)
        trues += [0.0] * int(lone.sum())
        scores += conf[lone].tolist()
      ap[0, li, oi] = _ap_of_curve(np.array(trues), np.array(scores), hard_fns) if trues else 0.0
  return ap


def cityscapes_ap_averages(ap):
  """computeAverages (:553-579) without distance terms: allAp = the mean over classes and overlaps that are not NaN, allAp50% the
  same at overlap 0.5, and per class 'ap' (the mean over the overlaps) and 'ap50%'."""
  import warnings
  import numpy as np
  with warnings.catch_warnings():
    warnings.simplefilter('ignore', RuntimeWarning)  # a mean over nothing but NaN is NaN, as in the script
    avg = {'allAp': float(np.nanmean(ap[0])), 'allAp50%': float(np.nanmean(ap[0, :, 0])), 'classes': {}}
  for li, (name, _) in enumerate(CITYSCAPES_LABELS):
    avg['classes'][name] = {'ap': float(np.average(ap[0, li, :])), 'ap50%': float(ap[0, li, 0])}
  return avg


def cityscapes_ap_result(records):
  """The dict of prepareJSONDataForResults (:644-654) for a list of match records."""
  ap = cityscapes_ap(records)
  return {'averages': cityscapes_ap_averages(ap), 'overlaps': _ap_overlaps().tolist(), 'minRegionSizes': list(AP_MIN_REGION_SIZES),
          'distanceThresholds': list(AP_DISTANCE_THS), 'minStereoDensities': list(AP_DISTANCE_CONFS),
          'instLabels': [n for n, _ in CITYSCAPES_LABELS], 'resultApMatrix': ap.tolist()}


def cityscapes_ap_table(averages):
  """printResults (:581-642) without colour codes and distance columns, as one string."""
  row = lambda what, a, b: '{:<15}'.format(what) + ':' + '{:>15.3f}'.format(a) + '{:>15.3f}'.format(b)
  lines = ['', '#' * 50, '{:<15}'.format('what') + ':' + '{:>15}'.format('AP') + '{:>15}'.format('AP_50%'), '#' * 50]
  lines += [row(name, averages['classes'][name]['ap'], averages['classes'][name]['ap50%']) for name, _ in CITYSCAPES_LABELS]
  lines += ['-' * 50, row('average', averages['allAp'], averages['allAp50%']), '']
  return '\n'.join(lines)


class CityscapesAPAnalyzer(object):
  """The scorer behind the output stage: AP and AP50% of the Cityscapes instance-level evaluation, from the masks while they
  are on the device.  names: as for RenderCityScapesOutputAnalyzer.  stage(results) takes what
  cityscapes_eval.iter_label_instances yields — 'y_out' [B,T,H,W], 'conf' [B,T], 'label_id' int32 [B,T] (-1 = not written),
  'indices' — plus 'gt_ids' int32 [B,H,W] on the device, runs the catalogue and the overlap kernel (once per 32 predictions; T
  itself is not limited) and keeps one match record per image (cityscapes_match_record); 'conf' and 'label_id' may also be host arrays (scores read from text files keep
  their float64 value that way).  finalize(path) evaluates all staged images, writes the result as JSON when given a path,
  prints the table and returns the dict.  One process: records of several ranks are not merged here."""

  def __init__(self, names):
    self.names = list(names)
    self.records = []  # (name, match record) per staged image

  def stage(self, results):
    import numpy as np
    y, gt = results['y_out'], results['gt_ids']
    indices = [int(i) for i in results['indices']]
    img_names = [str(self.names[i]) for i in indices]
    host = lambda a: a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    catalog = ops.gt_instance_catalog(gt, names=img_names)
    # the counts of one prediction do not depend on the others: more than the kernel's 32 go in several launches on one catalogue
    parts = [ops.instance_overlap(y[:, t0:t0 + ops.OVERLAP_MAX_T].contiguous(), gt, catalog)
             for t0 in range(0, y.shape[1], ops.OVERLAP_MAX_T)]
    inter, pred = (torch.cat(p, dim=1) for p in zip(*parts))
    ids, pixels, count = (host(t) for t in catalog)
    inter, pred, lab, conf = host(inter), host(pred), host(results['label_id']), host(results['conf'])
    for ii, name in enumerate(img_names):
      n = int(count[ii])
      self.records.append((name, cityscapes_match_record(ids[ii, :n], pixels[ii, :n], inter[ii, :, :n], pred[ii], lab[ii], conf[ii])))

  def finalize(self, path=None, quiet=False):
    import json
    result = cityscapes_ap_result([r for _, r in self.records])
    if path is not None:
      with open(path, 'w') as f:
        json.dump(result, f, indent=4, sort_keys=True)
    if not quiet:
      print(cityscapes_ap_table(result['averages']))
    return result


# ---- Cityscapes pixel-level evaluation (data_api/cityscapes_scripts/evaluation/evalPixelLevelSemanticLabeling.py) ----
# Line numbers below are that script's.  The pixel work (evaluatePair, :532-615: the confusion matrix and the true positives of
# every ground-truth instance) runs on the device (ops.pixel_confusion); what is left is a 34 x 34 integer matrix, two
# integers per instance, and float64 NumPy on those.
# helpers/labels.py as data: (id, name, category, hasInstances, ignoreInEval); its id -1 (license plate) cannot occur in an image
PIXEL_LABEL_TABLE = (
    (0, 'unlabeled', 'void', False, True), (1, 'ego vehicle', 'void', False, True),
    (2, 'rectification border', 'void', False, True), (3, 'out of roi', 'void', False, True),
    (4, 'static', 'void', False, True), (5, 'dynamic', 'void', False, True), (6, 'ground', 'void', False, True),
    (7, 'road', 'flat', False, False), (8, 'sidewalk', 'flat', False, False), (9, 'parking', 'flat', False, True),
    (10, 'rail track', 'flat', False, True), (11, 'building', 'construction', False, False),
    (12, 'wall', 'construction', False, False), (13, 'fence', 'construction', False, False),
    (14, 'guard rail', 'construction', False, True), (15, 'bridge', 'construction', False, True),
    (16, 'tunnel', 'construction', False, True), (17, 'pole', 'object', False, False), (18, 'polegroup', 'object', False, True),
    (19, 'traffic light', 'object', False, False), (20, 'traffic sign', 'object', False, False),
    (21, 'vegetation', 'nature', False, False), (22, 'terrain', 'nature', False, False), (23, 'sky', 'sky', False, False),
    (24, 'person', 'human', True, False), (25, 'rider', 'human', True, False), (26, 'car', 'vehicle', True, False),
    (27, 'truck', 'vehicle', True, False), (28, 'bus', 'vehicle', True, False), (29, 'caravan', 'vehicle', True, True),
    (30, 'trailer', 'vehicle', True, True), (31, 'train', 'vehicle', True, False), (32, 'motorcycle', 'vehicle', True, False),
    (33, 'bicycle', 'vehicle', True, False))
PIXEL_CATEGORIES = ('void', 'flat', 'construction', 'object', 'nature', 'sky', 'human', 'vehicle')  # in the table's order
PIXEL_AVG_CLASS_SIZE = {  # :135-146
    'bicycle': 4672.3249222261, 'caravan': 36771.8241758242, 'motorcycle': 6298.7200839748, 'rider': 3930.4788056518,
    'bus': 35732.1511111111, 'train': 67583.7075812274, 'car': 12794.0202738185, 'person': 3462.4756337644,
    'truck': 27855.1264367816, 'trailer': 16926.9763313609}
_PIXEL_STAT_KEYS = ('tp', 'tpWeighted', 'fn', 'fnWeighted')


def pixel_instance_stats():
  """generateInstanceStats (:171-202): zeroed tp / tpWeighted / fn / fnWeighted for every label that has instances and is
  evaluated, and for every category all of whose labels have instances (human, vehicle; 'labelIds' lists ALL its labels,
  caravan and trailer included)."""
  stats = {'classes': {}, 'categories': {}}
  for _, name, _, has_inst, ignore in PIXEL_LABEL_TABLE:
    if has_inst and not ignore:
      stats['classes'][name] = {k: 0.0 for k in _PIXEL_STAT_KEYS}
  for cat in PIXEL_CATEGORIES:
    rows = [r for r in PIXEL_LABEL_TABLE if r[2] == cat]
    if all(r[3] for r in rows):
      stats['categories'][cat] = dict({k: 0.0 for k in _PIXEL_STAT_KEYS}, labelIds=[r[0] for r in rows])
  return stats


def pixel_instance_stats_add(stats, ids, pixels, inst_tp, inst_cat_tp):
  """:581-615 for one image, from its catalogue (ids ascending, pixels) and the kernel's counts per slot: only ids > 1000 whose
  label is evaluated count, each with weight = avgClassSize / its size; the sums grow in the toolkit's order."""
  for inst_id, size, tp, cat_tp in zip(ids, pixels, inst_tp, inst_cat_tp):
    inst_id, size, tp, cat_tp = int(inst_id), int(size), int(tp), int(cat_tp)
    if inst_id <= 1000:
      continue
    label = inst_id // 1000
    if label >= len(PIXEL_LABEL_TABLE):
      raise ops.rn.RecAttendError('instance id %d: label %d is not a Cityscapes label (0 .. 33)' % (inst_id, label))
    _, name, cat, _, ignore = PIXEL_LABEL_TABLE[label]
    if ignore:
      continue
    weight = PIXEL_AVG_CLASS_SIZE[name] / float(size)
    for rec, t in ((stats['classes'][name], tp),) + (((stats['categories'][cat], cat_tp),) if cat in stats['categories'] else ()):
      rec['tp'] += t
      rec['fn'] += size - t
      rec['tpWeighted'] += float(t) * weight
      rec['fnWeighted'] += float(size - t) * weight


def _pixel_average(scores):
  """getScoreAverage (:273-282): the mean over the entries that are not NaN, NaN when there is none."""
  import math
  vals = [v for v in scores.values() if not math.isnan(v)]
  return sum(vals, 0.0) / len(vals) if vals else float('nan')


def cityscapes_pixel_scores(conf, inst_stats):
  """The scores of evalPixelLevelSemanticLabeling.py from conf [34,34] (conf[g][p] = pixels with ground-truth label g and
  predicted label p) and inst_stats (pixel_instance_stats, filled): classScores / classInstScores per label name (:216-265)
  and categoryScores / categoryInstScores per category (:285-338) — tp / (tp + fp + fn) in float64, where fp is the label's
  (category's) column(s) over the rows of labels that are evaluated and not the label itself (not in the category): pixels
  whose ground truth is ignored cost nothing; iIoU takes fp from the matrix and the weighted tp / fn from the instances.
  NaN for an ignored label, a label without instances (iIoU), a category without evaluated labels and for 0 / 0.  Plus
  the four averages (:273-282, :353-356) over the entries that are not NaN."""
  import numpy as np
  conf = np.asarray(conf).astype(np.int64)
  n = len(PIXEL_LABEL_TABLE)
  if conf.shape != (n, n):
    raise ops.rn.RecAttendError('cityscapes_pixel_scores: conf must be [%d,%d], got %s' % (n, n, conf.shape))
  nan = float('nan')
  evaluated = [r[0] for r in PIXEL_LABEL_TABLE if not r[4]]
  out = {k: {} for k in ('classScores', 'classInstScores', 'categoryScores', 'categoryInstScores')}
  for label, name, _, _, ignore in PIXEL_LABEL_TABLE:
    if ignore:
      out['classScores'][name] = out['classInstScores'][name] = nan
      continue
    tp = int(conf[label, label])
    fn = int(conf[label, :].sum()) - tp
    fp = int(conf[[l for l in evaluated if l != label], label].sum())
    out['classScores'][name] = float(tp) / (tp + fp + fn) if tp + fp + fn else nan
    rec = inst_stats['classes'].get(name)
    if rec is None:
      out['classInstScores'][name] = nan
    else:
      denom = rec['tpWeighted'] + fp + rec['fnWeighted']
      out['classInstScores'][name] = float(rec['tpWeighted']) / denom if denom != 0 else nan
  for cat in PIXEL_CATEGORIES:
    members = [r[0] for r in PIXEL_LABEL_TABLE if r[2] == cat and not r[4]]
    others = [r[0] for r in PIXEL_LABEL_TABLE if r[2] != cat and not r[4]]
    if not members:
      out['categoryScores'][cat] = nan
    else:
      tp = int(conf[np.ix_(members, members)].sum())
      fn = int(conf[members, :].sum()) - tp
      fp = int(conf[np.ix_(others, members)].sum())
      out['categoryScores'][cat] = float(tp) / (tp + fp + fn) if tp + fp + fn else nan
    rec = inst_stats['categories'].get(cat)
    if rec is None:
      out['categoryInstScores'][cat] = nan
    else:
      fp = int(conf[np.ix_(others, rec['labelIds'])].sum())  # :322,330: the columns of ALL the category's labels
      denom = rec['tpWeighted'] + fp + rec['fnWeighted']
      out['categoryInstScores'][cat] = float(rec['tpWeighted']) / denom if denom != 0 else nan
  out['averageScoreClasses'] = _pixel_average(out['classScores'])
  out['averageScoreInstClasses'] = _pixel_average(out['classInstScores'])
  out['averageScoreCategories'] = _pixel_average(out['categoryScores'])
  out['averageScoreInstCategories'] = _pixel_average(out['categoryInstScores'])
  return out


def cityscapes_pixel_result(conf, inst_stats):
  """The dict of writeJSONFile (:341-363) — confMatrix, priors, labels, the four score dicts and the four averages — plus
  averageScorePredictedClasses: the mean class IoU over the eight thing labels of CITYSCAPES_LABELS only.  The toolkit's
  averageScoreClasses runs over its 19 evaluated classes, of which the pre-stage predicts eight (the other eleven score 0
  wherever they occur in the ground truth), so only the extra key says how good the model is at what it does predict."""
  import numpy as np
  conf = np.asarray(conf).astype(np.int64)
  scores = cityscapes_pixel_scores(conf, inst_stats)
  total = int(conf.sum())
  result = {'confMatrix': conf.tolist(),
            'priors': {r[1]: (float(int(conf[r[0], :].sum())) / total if total else float('nan')) for r in PIXEL_LABEL_TABLE},
            'labels': {r[1]: r[0] for r in PIXEL_LABEL_TABLE}}
  result.update(scores)
  result['averageScorePredictedClasses'] = _pixel_average({n: scores['classScores'][n] for n, _ in CITYSCAPES_LABELS})
  return result


def cityscapes_pixel_table(result):
  """printClassScores / printCategoryScores (:416-440, :496-521) without colour codes, as one string."""
  row = lambda name, a, b: '{:<14}: '.format(name) + '{:>5.3f}'.format(a) + '    ' + '{:>5.3f}'.format(b)
  rule = '-' * 32
  lines = ['', 'classes          IoU      nIoU', rule]
  lines += [row(r[1], result['classScores'][r[1]], result['classInstScores'][r[1]]) for r in PIXEL_LABEL_TABLE if not r[4]]
  lines += [rule, row('Score Average', result['averageScoreClasses'], result['averageScoreInstClasses']), rule,
            row('Thing classes', result['averageScorePredictedClasses'], float('nan')), rule, '',
            'categories       IoU      nIoU', rule]
  lines += [row(c, result['categoryScores'][c], result['categoryInstScores'][c]) for c in PIXEL_CATEGORIES if c != 'void']
  lines += [rule, row('Score Average', result['averageScoreCategories'], result['averageScoreInstCategories']), rule, '']
  return '\n'.join(lines)


class CityscapesPixelAnalyzer(object):
  """Class IoU / iIoU of the Cityscapes pixel-level evaluation, from label images or the pre-stage's semantic map while they
  are on the device.  names: the file name of every image, indexed by results['indices'].  stage(results) takes 'gt_ids'
  int32 [B,H,W] (the *_gtFine_instanceIds.png values), optionally 'gt_labels' uint8 [B,H,W] (else the label is derived from
  the id), 'indices', and the prediction as 'pred' uint8 [B,H,W] or as 'sem' float32 [B,Hs,Ws,C] with 'size' = (H, W) — the
  fused form: the arg-max labels are never written.  It is the catalogue, ONE ops.pixel_confusion call into a device matrix
  that lives as long as the analyzer, and one small device-to-host copy (catalogue, per-instance counts, status words); the
  instance sums grow in the toolkit's order: images as staged, instances by ascending id.  finalize(path) checks the
  toolkit's sanity condition (the matrix sums to the pixels seen), writes the result (cityscapes_pixel_result) as JSON when
  given a path, prints the class table and returns the dict.  One process: several ranks are not merged here."""

  def __init__(self, names):
    self.names = list(names)
    self.conf = None  # int64 [34,34] on the device
    self.inst_stats = pixel_instance_stats()
    self.pixels = 0

  def stage(self, results):
    gt = results['gt_ids']
    img_names = [str(self.names[int(i)]) for i in results['indices']]
    fused = 'sem' in results
    ids, pixels, count, cstatus = ops.gt_instance_catalog(gt, check_status=False)
    out = ops.pixel_confusion(results['sem'] if fused else results['pred'], gt, results.get('gt_labels'), catalog=(ids, pixels, count),
                              size=results['size'] if fused else None, conf=self.conf, names=img_names, check_status=False)
    self.conf = out['conf']
    G = ops.MAX_GT
    host = torch.cat([ids, pixels, out['inst_tp'], out['inst_cat_tp'], count[:, None], cstatus[:, None], out['status'][:, None]],
                     dim=1).cpu().numpy()
    ops._raise_gt_status(torch.as_tensor(host[:, 4 * G + 1]), img_names, 'CityscapesPixelAnalyzer')
    ops._raise_pixel_status(host[:, 4 * G + 2], img_names, 'CityscapesPixelAnalyzer')
    for row in host:
      n = int(row[4 * G])
      pixel_instance_stats_add(self.inst_stats, row[:n], row[G:G + n], row[2 * G:2 * G + n], row[3 * G:3 * G + n])
    self.pixels += int(gt.shape[0]) * int(gt.shape[1]) * int(gt.shape[2])

  def finalize(self, path=None, quiet=False):
    import json
    import numpy as np
    conf = self.conf.cpu().numpy() if self.conf is not None else np.zeros((len(PIXEL_LABEL_TABLE),) * 2, np.int64)
    if int(conf.sum()) != self.pixels:  # :462-463, :472-473
      raise ops.rn.RecAttendError('Number of analyzed pixels and entries in confusion matrix disagree: confMatrix %d, pixels %d' % (
          int(conf.sum()), self.pixels))
    result = cityscapes_pixel_result(conf, self.inst_stats)
    if path is not None:
      with open(path, 'w') as f:
        json.dump(result, f, indent=4, sort_keys=True)
    if not quiet:
      print(cityscapes_pixel_table(result))
    return result


# ---------------------------------------------------------------------------- whole-dataset foreground / background IoU
def _fg_counts_of(results, index):
  """(count_a, sum_ab, sum_b, pixels) of one stage() call as Python integers: from results['fg_counts'] (what
  ops.fg_sweep_counts returns; `index` picks the threshold) or from binary device tensors results['y_out'] / results['y_gt']
  [N,H,W] ([N,T,H,W]: the maximum over T first, analysis.py:849-851)."""
  if 'fg_counts' in results:
    c = results['fg_counts']
    ca, sab = c['count_a'], c['sum_ab']
    n = len(c['sum_b'])
    pick = (lambda a: [int(v[index]) for v in a]) if getattr(ca, 'ndim', 2) == 2 else (lambda a: [int(v) for v in a])
    pix = c['pixels']  # one number for images of one size, or one per image (ops.fg_sweep_counts_ragged)
    return sum(pick(ca)), sum(pick(sab)), sum(int(v) for v in c['sum_b']), sum(int(v) for v in pix) if hasattr(pix, '__len__') else int(pix) * n
  a, b = results['y_out'], results['y_gt']
  if not (isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor) and a.is_cuda and b.is_cuda):
    raise ops.rn.RecAttendError('the whole-dataset IoU analyzers take results[\'fg_counts\'] or device tensors y_out / y_gt; '
                                'there is no CPU path')
  if a.dim() == 4:
    a, b = a.max(dim=1).values, b.max(dim=1).values
  if a.shape != b.shape or a.dim() != 3:
    raise ops.rn.RecAttendError('y_out %s and y_gt %s must both be [N,H,W] (or [N,T,H,W])' % (tuple(a.shape), tuple(b.shape)))
  a, b = a.to(torch.int64), b.to(torch.int64)
  return int(a.sum()), int((a * b).sum()), int(b.sum()), int(a.numel())


class ForegroundIOUAnalyzer(object):
  """analysis.py:834-867: IoU over an entire dataset, not per image — inter = sum a b, union = sum a + sum b - inter over every
  staged image, a the thresholded output and b the ground truth summed over the instances (b > 1 where instances overlap
  counts as a * b and b.sum() count it).  The sums are kept as exact Python integers; finalize() divides once in float64."""

  def __init__(self, name='FG IOU ALL', fname=None, index=0):
    self.name, self.fname, self.index = name, fname, index
    self.inter = self.union = 0

  def stage(self, results):
    count_a, sum_ab, sum_b, _ = _fg_counts_of(results, self.index)
    self.inter += sum_ab                     # :852
    self.union += count_a + sum_b - sum_ab   # :853

  def finalize(self):
    iou = self.inter / self.union if self.union else float('nan')  # :865 (0 / 0 there); integers: one rounding, float64
    print('{:17s}{:7.4f}'.format(self.name, iou))  # :866
    return iou


class BackgroundIOUAnalyzer(ForegroundIOUAnalyzer):
  """analysis.py:870-906: the same for the background, _a = 1 - a and _b = 1 - b, written out as it stands there: with b > 1
  the products (1 - a)(1 - b) are negative where a = 0, and so is what this returns."""

  def __init__(self, name='BG IOU ALL', fname=None, index=0):
    ForegroundIOUAnalyzer.__init__(self, name, fname, index)

  def stage(self, results):
    count_a, sum_ab, sum_b, pixels = _fg_counts_of(results, self.index)
    inter = pixels - count_a - sum_b + sum_ab                  # :891: sum (1 - a)(1 - b)
    union = (pixels - count_a) + (pixels - sum_b) - inter      # :892: sum _a + sum _b - inter
    self.inter += inter
    self.union += union
