"""analysis.py of the reference (the metric functions, :314-787) on the MI355X.

`results` is the dict full_model_eval.py:128-135 builds — 'y_out' (thresholded, [B,T,H,W]),
'y_gt', 's_out', 's_gt' — with float32 CUDA tensors.  All functions share one device pass
(ops.eval_metrics: pairwise intersections on the MFMA streaming kernel + one small metrics
kernel), cached on the dict.  Of the analyzers that render images or write CSV files (:52-311,
:790-900) only RenderCityScapesOutputAnalyzer (:196-267, the Cityscapes instance-level output) is built; the others are
out of scope."""
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


class RenderCityScapesOutputAnalyzer(object):
  """:196-267.  names: the file name of every image ('<run>_<seq>_<frame>...[.png]', what dataset.get_fname returns there),
  indexed by results['indices'].  stage() writes <folder>/<run>/<name>.txt — one line '<name>_<t:03d>.png <label_id> <score>'
  per written instance — and every written mask as an 8-bit PNG, (seg * 255).astype('uint8'); <run> is the name up to its
  first '_'.  As in the reference the text file is opened anew by every stage() call: with several thresholds sharing one
  folder the last one staged is what remains."""

  def __init__(self, folder, names):
    if folder is None:
      raise Exception('No output folder')
    self.folder = folder
    self.names = list(names)
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
          seg = (y_out[ii, jj] * 255).to(torch.uint8).cpu().numpy()
          png.write_gray8(os.path.join(runfolder, img_file), seg)
          text_file.write(cityscapes_line(img_file, lab_h[ii, jj], score[ii, jj]))
          lines.append((img_file, int(lab_h[ii, jj]), float(score[ii, jj])))
      self.written.append((text_fn, lines))

  def finalize(self):
    pass
