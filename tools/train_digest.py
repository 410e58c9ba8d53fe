#!/usr/bin/env python
"""Two optimisation steps of every trainer variant, as digests: per variant a fresh child under its own time limit runs the
smallest net the tests build for it and prints one line, the sha256 over (loss of step 1, gradient bucket after step 1, loss of
step 2, parameter bucket after step 2).  The kernels sum in a fixed order without atomics, so two trees whose host code issues
the same launches on the same librecattend.so print byte-identical dumps:

  python tools/train_digest.py --pkg OTHER/rec-attend-public_amd --lib rec-attend-public_amd/librecattend.so --out a.txt
  python tools/train_digest.py --out b.txt && cmp a.txt b.txt

--pkg: the Python package directory to import the trainers from (default: this tree's); --lib: the library to load (default: the
one beside the package).  Stops at the first child that ends abnormally (nothing more is started on the device) and returns its
status.  A variant whose digest differs between two runs of ONE tree is not deterministic and cannot be compared this way."""
import argparse
import hashlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

VARIANTS = ('full_stacked', 'full_per_timestep', 'full_bf16_operands', 'full_bf16_storage', 'full_filter_sizes', 'full_skip_stacked',
            'full_skip_per_timestep', 'box', 'fg_narrow', 'fg_wide')


def _full(variant):
  """(model, feed) of a full_model / box_model variant; the trainer is made here where the variant sets one of its switches."""
  import numpy as np
  import box_model
  import full_model
  import ra_oracle as ora
  import ra_train
  import train_filter_cases as tfc
  from test_train_gpu import _case
  extra = {}
  if variant == 'full_filter_sizes':  # train_any_filter: layers of size 1, 5 and 7, stride-2 dcnn layers at 3, 5 and 1
    opt, P, x, y_gt, s_gt = tfc.step_case()
  elif variant == 'box':
    opt, _, x, y_gt, s_gt = _case()
    P = ora.random_params(opt, 7, box_model=True)
    P = {k: (v * 0.6).astype(np.float32) if tfc.is_filter(k) else v for k, v in P.items()}
    extra['noise'] = np.random.RandomState(9).uniform(0, 0.3, (3, 2, 64, 64)).astype(np.float32)
  elif variant.startswith('full_skip'):  # skip connections into the decoder, a packed input of 13 channels (the padded map)
    H, W, T, B = 64, 128, 2, 2
    opt = ora.make_opt('kitti', H, W, T, base_learn_rate=1e-3, learn_rate_decay=0.96, steps_per_learn_rate_decay=5000)
    P = ora.random_params(opt, 32)
    P = {k: (v * 0.5).astype(np.float32) if tfc.is_filter(k) else v for k, v in P.items()}
    rng = np.random.RandomState(31)
    x = rng.rand(B, H, W, 3).astype(np.float32)
    extra = dict(d_in=np.eye(8, dtype=np.float32)[rng.randint(0, 8, (B, H, W))], y_in=ora.softmax(rng.randn(B, H, W, 1)).astype(np.float32))
    y_gt, s_gt = np.zeros((B, T, H, W), np.float32), np.ones((B, T), np.float32)
    y_gt[:, 0, 6:30, 8:40] = 1
    y_gt[:, 1, 36:56, 50:120] = 1
  else:
    opt, P, x, y_gt, s_gt = _case(wmul=0.6, T=2)
    if variant.startswith('full_bf16'):
      opt = dict(opt, compute_dtype='bf16')
  m = (box_model if variant == 'box' else full_model).get_model(opt).load_weights(P)
  m.trainer = (ra_train.BoxTrainStep if variant == 'box' else ra_train.TrainStep)(m)
  if variant.endswith('per_timestep'):
    m.trainer.batched_backward = False
  if variant == 'full_bf16_operands':
    m.trainer.bf16_storage = False
  feed = dict({'x': x, 'y_gt': y_gt, 's_gt': s_gt, 'phase_train': True, 'aug': False}, **extra)
  return m.trainer, lambda: m.run(['loss', 'train_step'], feed)[0]


def _fg(variant):
  import fg_model
  import fg_oracle as fo
  import ra_fg_train
  from test_fg_train_gpu import DRAWS, _dev, graph_batch, graph_opt
  from test_fg_train_wide_gpu import wide_opt
  wide = variant == 'fg_wide'
  opt = wide_opt(3, 'bce') if wide else graph_opt(3, True, 'iou')
  model = fg_model.get_model(opt).load_weights(fo.random_weights(opt, 31))
  ts = ra_fg_train.FgTrainStep(model, wide=True) if wide else ra_fg_train.FgTrainStep(model)
  x, y, d = (_dev(a) for a in graph_batch(3, True, 32))
  return ts, lambda: ts.run(x, y, d, draws=DRAWS)['loss']


def child(variant, pkg, lib):
  for p in (os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'oracle'), pkg):
    sys.path.insert(0, p)
  import numpy as np
  import torch
  import ra_native as rn
  if lib:
    rn.LIB_PATH = lib
  if not torch.cuda.is_available():
    raise SystemExit('train_digest: needs an MI355X')
  trainer, step = (_fg if variant.startswith('fg_') else _full)(variant)
  sha = hashlib.sha256()
  take = lambda t: sha.update(np.ascontiguousarray(t.detach().cpu().numpy()).tobytes())
  loss1 = step()
  take(torch.as_tensor(loss1))
  take(trainer.bucket.grad)
  loss2 = step()
  if hasattr(trainer, 'flush_status'):
    trainer.flush_status()
  take(torch.as_tensor(loss2))
  take(trainer.bucket.param)
  torch.cuda.synchronize()
  print('digest %s %s loss %.9g %.9g' % (variant, sha.hexdigest(), float(loss1), float(loss2)))


def main():
  ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
  ap.add_argument('--pkg', default=os.path.join(ROOT, 'rec-attend-public_amd'), help='the package directory to import the trainers from')
  ap.add_argument('--lib', help='the librecattend.so to run (default: the one beside the package)')
  ap.add_argument('--out')
  ap.add_argument('--timeout', type=int, default=150, help='seconds per variant')
  ap.add_argument('--case', choices=VARIANTS, help='run this one variant in this process (what the driver starts)')
  args = ap.parse_args()
  pkg, lib = os.path.abspath(args.pkg), os.path.abspath(args.lib) if args.lib else None
  if args.case:
    return child(args.case, pkg, lib)
  if not args.out:
    ap.error('--out is required')
  with open(args.out, 'w') as out:
    for variant in VARIANTS:
      cmd = ['timeout', '-k', '10', str(args.timeout), sys.executable, os.path.abspath(__file__), '--case', variant, '--pkg', pkg]
      r = subprocess.run(cmd + (['--lib', lib] if lib else []), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
      lines = [t for t in r.stdout.splitlines() if t.startswith('digest ')]
      if r.returncode != 0 or len(lines) != 1:
        sys.stdout.write(r.stdout)
        print('variant %s: the child ended with status %d; stopping' % (variant, r.returncode))
        return r.returncode if r.returncode > 0 else 1
      out.write(lines[0][len('digest '):] + '\n')
      out.flush()
      print(lines[0], flush=True)
  return 0


if __name__ == '__main__':
  sys.exit(main())
