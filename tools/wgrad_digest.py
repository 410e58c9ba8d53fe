#!/usr/bin/env python
"""The output bytes of every filter-gradient launch form, as digests: tests/wgrad_form_cases.py run once per RA_WGRAD_* variant
(A-F, each in a fresh child under its own time limit: the library reads the variables once per process), one line per variant,
case and shape.  Every kernel sums in a fixed order and uses no atomics, so two builds of librecattend.so compute the same
filter gradients exactly when their dumps are byte-identical:

  python tools/wgrad_digest.py --lib A/librecattend.so --out a.txt      # prints the line count and sha256 of a.txt
  python tools/wgrad_digest.py --lib B/librecattend.so --out b.txt && cmp a.txt b.txt

Stops at the first child that ends abnormally (nothing more is started on the device) and returns its status.
tools/ctrl_digest.py and tools/bn_digest.py run main() over the controller's and the BatchNorm case tables."""
import argparse
import hashlib
import importlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def main(cases='wgrad_form_cases', env_prefix='RA_WGRAD', doc=__doc__):
  """cases: the module under tests/ with VARIANTS, parse_line (and digest_text, where not all of a line is compared) and a runner
  that takes --lib; env_prefix: the variables its variants set"""
  ap = argparse.ArgumentParser(description=doc.split('\n')[0])
  ap.add_argument('--lib', help='the librecattend.so to run (default: the tree\'s own)')
  ap.add_argument('--out', required=True)
  ap.add_argument('--timeout', type=int, default=120, help='seconds per variant')
  args = ap.parse_args()
  wf = importlib.import_module(cases)
  cmd = ['timeout', '-k', '10', str(args.timeout), sys.executable, os.path.join(ROOT, 'tests', cases + '.py')]
  if args.lib:
    cmd += ['--lib', os.path.abspath(args.lib)]
  base = {k: v for k, v in os.environ.items() if not k.startswith(env_prefix)}
  sha, lines = hashlib.sha256(), 0
  with open(args.out, 'wb') as out:
    for variant, env in wf.VARIANTS.items():
      r = subprocess.run(cmd, env=dict(base, **env), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
      if r.returncode != 0:
        sys.stdout.write(r.stdout)
        print('variant %s: the runner ended with status %d; stopping' % (variant, r.returncode))
        return r.returncode if r.returncode > 0 else 1
      for text in r.stdout.splitlines():
        if wf.parse_line(text) is None:
          continue
        line = ('%s %s\n' % (variant, getattr(wf, 'digest_text', str)(text))).encode()
        out.write(line)
        sha.update(line)
        lines += 1
  print('%s: %d lines, sha256 %s' % (args.out, lines, sha.hexdigest()))
  return 0


if __name__ == '__main__':
  sys.exit(main())
