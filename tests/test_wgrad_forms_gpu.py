"""The filter-gradient kernels on the paths no other test reaches: several tiles per workgroup (the persistent walk, the register
prefetch across tiles, the LDS double buffer of the DMA forms), the 16-block form, and the generic kernel with its prefetch or
its packed rows switched off.  The RA_WGRAD_* variables that select them are read once per process, so each variant of
tests/wgrad_form_cases.py runs the whole case table in a fresh child; variant A (nothing set) is what the rest of the suite
runs under.  Bars: the project's own, stated beside the cases."""
import os
import subprocess
import sys

import pytest

import wgrad_form_cases as wf

pytestmark = pytest.mark.gpu

TIME_LIMIT = 120  # seconds per child: a few of start-up, the launches themselves are microseconds
_broken = []      # the variant whose child ended with a non-zero status or at its time limit: nothing more is started after it


@pytest.mark.parametrize('variant', ['B', 'C', 'E', 'F'])
def test_wgrad_forms(cuda, variant):
  assert not _broken, 'not started: the child of variant %s ended abnormally' % _broken[0]
  env = {k: v for k, v in os.environ.items() if not k.startswith('RA_WGRAD')}
  env.update(wf.VARIANTS[variant])
  try:
    r = subprocess.run([sys.executable, wf.__file__], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=TIME_LIMIT)
  except subprocess.TimeoutExpired as e:
    _broken.append(variant)
    raise AssertionError('variant %s: no end after %d s\n%s' % (variant, TIME_LIMIT, e.stdout))
  print(r.stdout)
  if r.returncode != 0:  # the runner never exits non-zero over an error bar: a signal, an abort or a HIP error that rn.check reported
    _broken.append(variant)
  assert r.returncode == 0, 'variant %s: the runner ended with status %d\n%s' % (variant, r.returncode, r.stdout)
  rows = [p for p in map(wf.parse_line, r.stdout.splitlines()) if p is not None]
  assert len(rows) == len(wf.CASES) * len(wf.SHAPES), (len(rows), r.stdout)
  bad = [(name, err, bar) for name, _, errs in rows for err, bar in errs if not err < bar]
  assert not bad, bad
