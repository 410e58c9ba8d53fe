#!/usr/bin/env python
"""The output bytes of every controller form, as digests: tests/ctrl_form_cases.py run once per RA_CTRL_XCD variant (each in a
fresh child under its own time limit: the library reads the variable once per process), one line per variant, case and form.  No
controller kernel uses float atomics and every sum has a fixed order, so two builds of librecattend.so compute the same
controller outputs exactly when their dumps are byte-identical:

  python tools/ctrl_digest.py --lib A/librecattend.so --out a.txt && python tools/ctrl_digest.py --out b.txt && cmp a.txt b.txt

The driver is tools/wgrad_digest.py's: it stops at the first child that ends abnormally and returns its status."""
import sys

import wgrad_digest

if __name__ == '__main__':
  sys.exit(wgrad_digest.main('ctrl_form_cases', 'RA_CTRL_XCD', __doc__))
