"""The controller kernels under every setting of RA_CTRL_XCD: the default, the agent-scope exchange for every form (0: no other
test runs it for the per-image form at B <= 8, or for the group-shared form with an XCD offset given) and the XCD-local per-image
form with two teams on an XCD (2, B = 11).  The variable is read once per process, so each variant of tests/ctrl_form_cases.py
runs the whole case table in a fresh child.  Bars: those of tests/test_kernels_gpu.py, stated in the runner; the status word of
every case must be 0.  Every spin loop of the kernels is bounded (kSpinLimit), so a starved team shows as status 1: a failure to
diagnose from the code, not to run again.

The library has no query for the exchange a launch ran, so this test cannot tell that a variant's variable took effect: were
RA_CTRL_XCD ignored, the three children would run the same code and pass.  What shows it is the timing (tools/ctrl_forms.py:
the agent-scope per-image form is about 6 us a launch slower at cfg2) and ra_ctrl_split.hip's xcd_local(), the one place
that reads the variable."""
import os
import subprocess
import sys

import pytest

import ctrl_form_cases as cf

pytestmark = pytest.mark.gpu

TIME_LIMIT = 120  # seconds per child: a few of start-up and the float64 references, the launches themselves are microseconds
_broken = []      # the variant whose child ended with a non-zero status or at its time limit: nothing more is started after it


@pytest.mark.parametrize('variant', list(cf.VARIANTS))
def test_ctrl_forms(cuda, variant):
  assert not _broken, 'not started: the child of variant %s ended abnormally' % _broken[0]
  env = {k: v for k, v in os.environ.items() if k != 'RA_CTRL_XCD'}
  env.update(cf.VARIANTS[variant])
  try:
    r = subprocess.run([sys.executable, cf.__file__], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=TIME_LIMIT)
  except subprocess.TimeoutExpired as e:
    _broken.append(variant)
    raise AssertionError('variant %s: no end after %d s\n%s' % (variant, TIME_LIMIT, e.stdout))
  print(r.stdout)
  if r.returncode != 0:  # the runner never exits non-zero over an error bar: a signal, an abort, a HIP error, or a status word that is not 0
    _broken.append(variant)
  assert r.returncode == 0, 'variant %s: the runner ended with status %d\n%s' % (variant, r.returncode, r.stdout)
  rows = [p for p in map(cf.parse_line, r.stdout.splitlines()) if p is not None]
  assert [name for name, _, _, _ in rows] == cf.case_names(), r.stdout
  assert all(status == 0 for _, _, status, _ in rows)
  bad = [(name, err, bar) for name, _, _, errs in rows for err, bar in errs if not err < bar]
  assert not bad, bad
