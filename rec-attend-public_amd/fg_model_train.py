#!/usr/bin/env python
"""Entry point with the flag surface of the reference's fg_model_train.py (:425-448 + TrainArgsParser + DataArgsParser):
trains the pre-stage fg_model — step two of run_kitti.sh / run_cityscapes.sh, between the label stage and fg_model_pack.py —
by default for nets whose layers have up to 128 output channels (ra_fg_train.FgTrainStep; wider nets are refused by name).
--train_wide opts into the wide path (layers of up to 512 output channels, inputs of up to 1024: the nets of run_kitti.sh and
run_cityscapes.sh); the flag is saved in model_opt.yaml as train_wide, so that --restore continues on the same path, and
fg_model_pack.py / fg_model_eval.py ignore it.  It is a flag and not the default because the suite pins the default's refusals
(ra_fg_train's docstring).

--input is an .npz with x [N,h,w,3], y_gt [N,h,w] or [N,h,w,nsc] and, with --add_orientation, d_gt [N,h,w,8]: exactly what
`setup_labels.py --target fg_model` writes.  Batch k takes the images (k * batch_size + i) % N.  --valid_input (optional, the
same layout) is scored with fg_model.Model.statistics every --steps_per_valid steps, the means over its batches as the
reference's Evaluator averages them.

Writes <results>/<model_id>/model_opt.yaml, weights.npz (the checkpoint names of fg_model.save_var_names plus `step`: what
fg_model_pack.py --model_id and fg_model_eval.py --model_id restore), optimizer.npz (ra_fg_train.FgTrainStep.state_dict) and
log.txt, one line per logged step; every --steps_per_ckpt steps under --save_ckpt, and when the run ends.  --restore <folder>
continues from that folder's weights.npz and optimizer.npz at its global step.  The reference's HDF5 reader and its plots are
out of scope."""
import argparse
import os
import time

import numpy as np
import yaml

import cmd_args_parser as cap
from ra_native import RecAttendError

LOGGED = ('loss', 'foreground_loss', 'iou_soft', 'iou_hard', 'orientation_ce', 'orientation_acc')


def build_parser():
  p = argparse.ArgumentParser(description='Train the fg_model pre-stage')
  for table in (cap.TRAIN_FLAGS, cap.DATA_FLAGS, cap.FG_MODEL_FLAGS):
    cap.add_flags(p, table)
  p.add_argument('--input', default=None, help='.npz with x, y_gt (+ d_gt with --add_orientation)')
  p.add_argument('--valid_input', default=None, help='.npz of the same layout, scored every --steps_per_valid steps')
  p.add_argument('--seed', type=int, default=1234)
  p.add_argument('--train_wide', action='store_true', help='train layers of more than 128 channels (float32, uncaptured; '
                 'ra_fg_train.FgTrainStep(model, wide=True))')
  return p


def make_opt(args):
  opt = cap.make_fg_model_opt(args)
  opt['seed'] = int(args.seed)
  if getattr(args, 'train_wide', False):  # only when asked for: without the flag model_opt.yaml is what it was
    opt['train_wide'] = True
  return opt


def _load_archive(path, opt, what):
  data = np.load(path, allow_pickle=False)
  need = ('x', 'y_gt') + (('d_gt',) if opt['add_orientation'] else ())
  for k in need:
    if k not in data:
      raise RecAttendError('%s %s lacks %s (an .npz with %s, as setup_labels.py --target fg_model writes)' % (
          what, path, k, ', '.join(need)))
  out = {k: np.asarray(data[k], dtype=np.float32) for k in need}
  n = out['x'].shape[0]
  if n == 0 or any(v.shape[0] != n for v in out.values()):
    raise RecAttendError('%s %s: %s differ in their first dimension' % (what, path, ', '.join(need)))
  return out


def save(folder, model, trainer, model_opt):
  """model_opt.yaml, weights.npz and optimizer.npz, each written beside and renamed."""
  os.makedirs(folder, exist_ok=True)
  state = trainer.state_dict()  # looks at the last step's status word first
  with open(os.path.join(folder, 'model_opt.yaml'), 'w') as f:
    yaml.safe_dump(model_opt, f)
  weights = dict(model.state_dict_numpy(), step=np.asarray(float(trainer.bucket.global_step), dtype=np.float32))
  for name, arrays in (('weights.npz', weights), ('optimizer.npz', state)):
    tmp = os.path.join(folder, name + '.tmp.npz')
    np.savez(tmp, **arrays)
    os.replace(tmp, os.path.join(folder, name))


def validate(model, trainer, data, batch_size, up):
  trainer.sync_model()
  stats = []
  n = data['x'].shape[0]
  for b0 in range(0, n, batch_size):
    sl = slice(b0, min(n, b0 + batch_size))
    stats.append(model.statistics(up(data['x'][sl]), up(data['y_gt'][sl]), up(data['d_gt'][sl]) if 'd_gt' in data else None))
  return {k: float(np.mean([s[k] for s in stats])) for k in LOGGED if k in stats[0]}


def main(argv=None):
  import torch
  args = build_parser().parse_args(argv)
  if args.model_id is None:
    raise Exception('You must provide model ID')
  if args.input is None:
    raise RecAttendError('--input is required: an .npz with x, y_gt (+ d_gt), as setup_labels.py --target fg_model writes')
  if args.batch_size < 1 or args.num_steps < 0:
    raise RecAttendError('--batch_size %d, --num_steps %d' % (args.batch_size, args.num_steps))
  import fg_model
  import ra_fg_train
  model_opt = make_opt(args)
  folder = os.path.join(args.results, args.model_id)
  restore = args.restore
  if restore:  # the net is the restored run's, as fg_model_pack.restore_model reads it
    with open(os.path.join(restore, 'model_opt.yaml')) as f:
      model_opt = yaml.safe_load(f)
  model = fg_model.get_model(model_opt)
  if restore:
    model.load_weights(dict(np.load(os.path.join(restore, 'weights.npz'))))
  trainer = ra_fg_train.FgTrainStep(model, wide=bool(model_opt.get('train_wide', False)))  # refuses what is not built, and a machine without a device, before any data is read
  if restore:
    trainer.load_state_dict(dict(np.load(os.path.join(restore, 'optimizer.npz'))))
    print('restored %s at global_step %d' % (restore, trainer.bucket.global_step))
  data = _load_archive(args.input, model_opt, '--input')
  valid = _load_archive(args.valid_input, model_opt, '--valid_input') if args.valid_input and not args.no_valid else None
  dev = torch.device('cuda', torch.cuda.current_device())
  up = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
  n = data['x'].shape[0]
  os.makedirs(folder, exist_ok=True)
  log = open(os.path.join(folder, 'log.txt'), 'a')

  def emit(line):
    print(line)
    log.write(line + '\n')
    log.flush()

  t0 = time.time()
  start = trainer.bucket.global_step
  for step in range(start, args.num_steps):
    trainer.aug_gen.manual_seed((int(args.seed) + 104729 * step) % (2 ** 31 - 1))  # the draws are a function of the step
    idx = (step * args.batch_size + np.arange(args.batch_size)) % n
    out = trainer.run(up(data['x'][idx]), up(data['y_gt'][idx]), up(data['d_gt'][idx]) if 'd_gt' in data else None)
    if step % max(1, args.steps_per_log) == 0 or step == args.num_steps - 1:
      emit('step %d  %s  learn_rate %.2e  %.2f s' % (step, '  '.join('%s %.5f' % (k, float(out[k])) for k in LOGGED if k in out),
                                                    out['learn_rate'], time.time() - t0))
    if valid is not None and (step + 1) % max(1, args.steps_per_valid) == 0:
      v = validate(model, trainer, valid, args.batch_size, up)
      emit('step %d  valid  %s' % (step, '  '.join('%s %.5f' % kv for kv in v.items())))
    if args.save_ckpt and (step + 1) % max(1, args.steps_per_ckpt) == 0:
      save(folder, model, trainer, model_opt)
  trainer.flush_status()
  save(folder, model, trainer, model_opt)
  emit('trained to step %d, weights -> %s (model_opt.yaml, weights.npz, optimizer.npz)' % (trainer.bucket.global_step, folder))
  log.close()
  return trainer


if __name__ == '__main__':
  main()
