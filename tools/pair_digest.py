#!/usr/bin/env python
"""The output bytes of every fused-pair launch form, as digests: tests/pair_form_digest.py run once per RA_PAIR* variant (the
default dispatch, the persistent shapes on the one-shot kernel, the N-packed shapes on the generic pair, the cached kernel
with its float32 layer B), each in a fresh child under its own time limit, one line per variant and case.  No pair kernel
uses atomics on its results and every sum has a fixed order, so two builds of librecattend.so compute the same outputs, caches
and rider fills exactly when their dumps are byte-identical:

  python tools/pair_digest.py --lib A/librecattend.so --out a.txt && python tools/pair_digest.py --out b.txt && cmp a.txt b.txt

The driver is tools/wgrad_digest.py's: it stops at the first child that ends abnormally and returns its status."""
import sys

import wgrad_digest

if __name__ == '__main__':
  sys.exit(wgrad_digest.main('pair_form_digest', 'RA_PAIR', __doc__))
