#!/usr/bin/env python
"""Reduce the output of `python -m pytest tests/test_attn_geometry_gpu.py -q -m gpu -s` (one or more logs) to one line per shape,
entry point and geometry class: the worst error the GPU run measured over its tolerance, beside E32 / tolerance — the same
dense operator in float32 against float64 on the host, i.e. how much of the tolerance the reference's own conditioning takes —
and the paste plans the case ran (profiles/attn_geometry.txt)."""
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ('rec-attend-public_amd', 'oracle', 'tests'):
  sys.path.insert(0, os.path.join(ROOT, p))
import attn_geometry_cases as ag  # noqa: E402

LINE = re.compile(r'ATTN_GEOMETRY (\S+) (\S+) plans=(\S+) (.*)')
OPERATOR = {'extract_direct': 'extract', 'extract_conv0.patch': 'extract', 'paste_direct': 'paste', 'paste_score_direct': 'paste',
            'attn_box_direct': 'box', 'gaussian_filter': 'bank', 'resample_bwd': 'adjoint'}


def _per_record(a):
  return np.abs(a).reshape(a.shape[0], -1).max(axis=1)


def _by_class(pairs, ratio):
  out = {}
  for p, r in zip(pairs, ratio):
    for c in set(p):
      out[c] = max(out.get(c, 0.0), float(r))
  return out


def e32(sid):
  """operator -> class -> E32 / tolerance on the host."""
  if sid in ag.ADJOINT_SHAPES:
    import torch
    case = ag.adjoint_case(sid)
    n = case['rec'].shape[0]
    ex, _ = ag.adjoint_excess(ag.adjoint_reference(case, 0, n, torch.float32)[1], ag.adjoint_reference(case, 0, n, torch.float64)[1])
    return {'adjoint': _by_class(case['pairs'], ex)}
  ref = ag.reference(sid)
  H, W, Fh, Fw = ag.all_shapes()[sid]
  fy, fx = ag.dense_banks(ref['rec'], H, W, Fh, Fw)
  got = (ag.extract_op(ref['img_cv'], fy, fx), ag.paste_op(ref['P'], fy, fx, ref['rec']), ag.box_op(fy, fx, ref['rec']))
  tols = (ag.TOL_EXTRACT * np.maximum(1.0, _per_record(ref['extract'])), ag.TOL_PASTE, ag.TOL_BOX)
  out = {name: _by_class(ref['pairs'], _per_record(g - ref[name]) / tol) for name, g, tol in zip(('extract', 'paste', 'box'), got, tols)}
  out['bank'] = {}
  for axis, (b32, b64) in enumerate(((fy, ref['fy']), (fx, ref['fx']))):   # a bank belongs to its own axis' class
    ratio = _per_record(b32 - b64) / np.maximum(1e-6, _per_record(b64)) / 1e-4
    for c, r in _by_class([(p[axis],) for p in ref['pairs']], ratio).items():
      out['bank'][c] = max(out['bank'].get(c, 0.0), r)
  return out


def main(logs):
  rows, cache = [], {}
  for log in logs:
    for line in open(log):
      m = LINE.search(line)
      if m:
        rows.append((m.group(1), m.group(2), m.group(3), dict(kv.split('=') for kv in m.group(4).split())))
  print('%-8s %-28s %-17s %-9s %-9s %s' % ('shape', 'entry point', 'class', 'GPU/tol', 'E32/tol', 'paste plans'))
  for sid, entry, plans, by_class in rows:
    cache.setdefault(sid, e32(sid))
    op = OPERATOR.get(entry.split('.')[0] if entry.startswith('paste') else entry)
    for c in ag.CLASS_IDS:
      if c in by_class:
        ref = cache[sid].get(op, {}).get(c)
        print('%-8s %-28s %-17s %-9s %-9s %s' % (sid, entry, c, by_class[c], '-' if ref is None else '%.3f' % ref, plans.replace('|', ', ').replace('_', ' ')))
  print('%d cases' % len(rows))


if __name__ == '__main__':
  main(sys.argv[1:])
