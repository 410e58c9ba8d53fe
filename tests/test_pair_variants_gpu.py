"""The fused-pair kernels on the paths the default dispatch never takes a test to: the persistent shapes through the one-shot
kernel, the N-packed shapes (canvas plane included) through the generic pair, and the cached kernel with layer B on the float32
MFMA.  The RA_PAIR* variables that select them are read once per process, so each variant of tests/pair_form_digest.py walks
the whole case table in a fresh child, under --check: every output against the float64 oracle at test_pair_forms' bar.  The
default variant is what test_conv_forms_gpu.py::test_pair_forms runs."""
import os
import re
import subprocess
import sys

import pytest

import pair_form_digest as pf

pytestmark = pytest.mark.gpu

TIME_LIMIT = 180  # seconds per child: start-up, 144 small launches and their float64 references
_broken = []      # the variant whose child ended with a non-zero status or at its time limit: nothing more is started after it


@pytest.mark.parametrize('variant', [v for v in pf.VARIANTS if v != 'default'])
def test_pair_variant(cuda, variant):
  assert not _broken, 'not started: the child of variant %s ended abnormally' % _broken[0]
  env = {k: v for k, v in os.environ.items() if not k.startswith('RA_PAIR')}
  env.update(pf.VARIANTS[variant])
  r = subprocess.run(['timeout', '-k', '10', str(TIME_LIMIT), sys.executable, pf.__file__, '--check'], env=env, stdout=subprocess.PIPE,
                     stderr=subprocess.STDOUT, text=True)
  print(r.stdout)
  if r.returncode != 0:  # an error bar missed, or a signal, an abort, the time limit, a HIP error
    _broken.append(variant)
  assert r.returncode == 0, 'variant %s: the runner ended with status %d\n%s' % (variant, r.returncode, r.stdout)
  total, cached = len(pf.cases()), pf.n_cache_form()
  m = re.search(r'^ran (\d+) of (\d+) cases', r.stdout, re.M)
  assert m, r.stdout
  assert (int(m.group(1)), int(m.group(2))) == (total - cached if variant == 'no8' else total, total), m.group(0)
  rows = [p for p in map(pf.parse_line, r.stdout.splitlines()) if p is not None]
  assert len(rows) == int(m.group(1)) and all('err' in fields for _, fields, _ in rows)
