#!/usr/bin/env python
"""Every conv plan query over the coverage grids, one line per argument row: the query, its arguments, the return code, all
RA_PLAN_INTS ints of the record, and the error text of a refusal.  Two builds of librecattend.so choose the same launch forms
(and, on a device, the same grids, walks and tickets) exactly when their dumps are byte-identical:

  python tools/conv_plan_dump.py --lib A/librecattend.so --out a.txt      # prints the line count and sha256 of a.txt
  python tools/conv_plan_dump.py --lib B/librecattend.so --out b.txt && cmp a.txt b.txt

Without a device only the queries that need none are dumped (K1 and the pair; --all forces the rest).  The K1 rows are the
coverage test's, and the same with a canvas plane, with a second source (C1 = C0) and, for the bf16 kinds, store_flags 1-3."""
import argparse
import ctypes
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ('rec-attend-public_amd', 'tests'):
  sys.path.insert(0, os.path.join(ROOT, p))


def k1_rows(cf, cov):
  for kind, kw in cf.K1_KINDS.items():
    for row in cov._k1_rows(kind):
      yield row
      yield row[:9] + (1,) + row[10:]            # has_plane
      yield (row[0], row[0]) + row[2:]           # C1 = C0
      for flags in (1, 2, 3) if kw.get('bf16') else ():
        yield row[:12] + (flags,)


def main():
  ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
  ap.add_argument('--lib', help='the librecattend.so to ask (default: the tree\'s own)')
  ap.add_argument('--out', required=True)
  ap.add_argument('--all', action='store_true', help='also the device-following queries when no device is present')
  args = ap.parse_args()
  import ra_native as rn
  if args.lib:
    rn.LIB_PATH = os.path.abspath(args.lib)
  import conv_form_cases as cf
  import test_conv_forms_coverage as cov
  import torch
  grid = [(B, H, W) for B in cf.COVER_B for H in cf.COVER_HW for W in cf.COVER_HW]
  queries = [('conv3x3', k1_rows(cf, cov)), ('conv_pair', cov.pair_rows())]
  if args.all or torch.cuda.is_available():
    queries += [
        ('conv_split', ((B, H, W, ci, co, pool, plane) for B, H, W in grid for ci, co in cf.SPLIT_CHANNELS for pool in (1, 2) for plane in (0, 1))),
        ('conv_wino', ((B, H, W, ci, co, pool) for B, H, W in grid for ci, co in cf.WINO_CHANNELS for pool in (1, 2))),
        ('conv_pair_wino', iter(grid)),
    ]
  lib, rec, sha, lines = rn.lib(), (ctypes.c_int * rn.RA_PLAN_INTS)(), hashlib.sha256(), 0
  with open(args.out, 'wb') as out:
    for name, rows in queries:
      fn = getattr(lib, 'ra_%s_plan' % name)
      for row in rows:
        rc = fn(*row, rec)
        err = ' ' + (lib.ra_last_error_string() or b'').decode() if rc else ''
        line = ('%s %s -> %d : %s%s\n' % (name, ' '.join(map(str, row)), rc, ' '.join(map(str, rec)), err)).encode()
        out.write(line)
        sha.update(line)
        lines += 1
  print('%s: %d lines, sha256 %s' % (args.out, lines, sha.hexdigest()))


if __name__ == '__main__':
  main()
