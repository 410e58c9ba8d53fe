#!/usr/bin/env python
"""Entry point in the place of the reference's fg_model_pack.py (:1-71): runs the fg_model pre-stage over a set of images
and stores what the decode loop reads beside them.

Restores results/<model_id>/{model_opt.yaml, weights.npz} (checkpoint names of fg_model.get_save_var), feeds
{x, phase_train=False} batch by batch on the MI355X kernels and writes --output = the arrays of --input plus
y_in [N,H,W,nsc] and d_in [N,H,W,8]: y_out / d_out after the 8-bit round trip of the reference (fg_model_pack.py:41-48 writes
(v * 255).astype('uint8') PNGs, data_api/ins_seg_dataset.py:273-292 reads them back as uint8 / 255), as float32.  That
file is a valid --input of full_model_eval.py.  The reference's HDF5 datasets and PNG files are out of scope."""
import argparse
import os

import numpy as np
import yaml

import fg_model


def build_parser():
  p = argparse.ArgumentParser(description='Pack fg_model output')
  p.add_argument('--model_id', default=None)            # cmd_args_parser.py: EvalArgsParser
  p.add_argument('--results', default='../results')
  p.add_argument('--batch_size', default=10, type=int)
  p.add_argument('--input', required=True, help='.npz with x [N,H,W,3]')
  p.add_argument('--output', required=True, help='.npz to write: the input arrays plus y_in, d_in')
  return p


def restore_model(results, model_id):
  restore = os.path.join(results, model_id)
  with open(os.path.join(restore, 'model_opt.yaml')) as f:
    model_opt = yaml.safe_load(f)
  return fg_model.get_model(model_opt).load_weights(dict(np.load(os.path.join(restore, 'weights.npz'))))


def main(argv=None):
  import torch
  args = build_parser().parse_args(argv)
  if args.model_id is None:
    raise Exception('You must provide model ID')  # cmd_args_parser.py:154-155
  model = restore_model(args.results, args.model_id)
  data = dict(np.load(args.input))
  x = data['x']
  ys, ds = [], []
  for b0 in range(0, x.shape[0], max(1, args.batch_size)):
    y, d = model.prestage(x[b0:b0 + max(1, args.batch_size)], quantise=True)
    ys.append(y.cpu().numpy())
    if d is not None:
      ds.append(d.cpu().numpy())
  torch.cuda.synchronize()
  data['y_in'] = np.concatenate(ys)
  if ds:
    data['d_in'] = np.concatenate(ds)
  np.savez_compressed(args.output, **data)
  print('%d images -> %s (y_in %r%s)' % (x.shape[0], args.output, data['y_in'].shape,
                                         ', d_in %r' % (data['d_in'].shape,) if ds else ''))


if __name__ == '__main__':
  main()
