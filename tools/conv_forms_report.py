#!/usr/bin/env python
"""Reduce the output of `python -m pytest tests/test_conv_forms_gpu.py -q -m gpu -s` to one line per launch form: the case that
reaches it and the worst error it measured against the float64 oracle, beside the bar (profiles/conv_forms.txt)."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ('rec-attend-public_amd', 'tests'):
  sys.path.insert(0, os.path.join(ROOT, p))
import conv_form_cases as cf  # noqa: E402

LINE = re.compile(r'(K1 \w+|pair|K1s|Winograd pair|Winograd) (\(.*?\))( [^:]*)?: ([0-9.e+-]+) of the output scale \(bar ([0-9.e+-]+)\)')


def main(log):
  errs = {}  # (label, shape) -> [(what, err, bar)]
  for line in open(log):
    m = LINE.search(line)
    if m:
      errs.setdefault((m.group(1), m.group(2)), []).append(((m.group(3) or '').strip(), float(m.group(4)), float(m.group(5))))
  tables = [('K1 %s' % k, s, p, None) for k, s, p in cf.K1_CASES + cf.K1_EXTRA_CASES]
  for label, plain, walks in (('pair', cf.PAIR_CASES, cf.PAIR_WALK_CASES), ('K1s', cf.SPLIT_CASES, cf.SPLIT_WALK_CASES),
                              ('Winograd', cf.WINO_CASES, cf.WINO_WALK_CASES), ('Winograd pair', cf.PAIR_WINO_CASES, cf.PAIR_WINO_WALK_CASES)):
    tables += [(label, s, p, None) for s, p in plain] + [(label, s, p, w) for s, p, w in walks]
  print('%-14s %-44s %-78s %s' % ('entry', 'case', 'plan', 'worst error / bar'))
  missing = 0
  for label, shape, plan, walk in tables:
    got = errs.get((label, repr(shape)))
    if not got:
      missing += 1
      continue
    figs = ', '.join('%.2e / %.0e%s' % (e, b, ' (%s)' % w if w else '') for w, e, b in got)
    tail = '  walk (ntiles, grid, min, max) = %r' % (walk,) if walk else ''
    print('%-14s %-44s %-78s %s%s' % (label, repr(shape).replace(' ', ''), plan, figs, tail))
  print('%d cases, %d without a figure in the log' % (len(tables), missing))


if __name__ == '__main__':
  main(sys.argv[1])
