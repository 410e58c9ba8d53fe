#!/usr/bin/env python
"""The output bytes of every BatchNorm form, as digests: tests/bn_form_cases.py run in a fresh child under its own time limit,
one line per case (without the column of forms, which a build from before ra_bn_form cannot report).  No BatchNorm kernel uses
atomics and every sum has a fixed order, so two builds of librecattend.so compute the same moments, activations and gradients
exactly when their dumps are byte-identical:

  python tools/bn_digest.py --lib A/librecattend.so --out a.txt && python tools/bn_digest.py --out b.txt && cmp a.txt b.txt

The driver is tools/wgrad_digest.py's: it stops at the first child that ends abnormally and returns its status."""
import sys

import wgrad_digest

if __name__ == '__main__':
  sys.exit(wgrad_digest.main('bn_form_cases', 'RA_BN', __doc__))
