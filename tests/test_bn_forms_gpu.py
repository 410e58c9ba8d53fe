"""The train-mode BatchNorm kernels in every form the chooser of csrc/ra_bn.hip selects, at the smallest shapes that reach
each path: tests/bn_form_cases.py's table, run in this process (no variable selects a form, so there are no variants).  Each
case asserts the form ra_bn_form reports for every pass against the case's literals, the float64 oracle's bars stated beside
the table, and the bit-for-bit relations between the entry points (accumulating, split, grouped, bf16 storage, refusals)."""
import pytest
import torch

import bn_form_cases as bf
import ra_native as rn

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('case', bf.CASES, ids=[c['name'] for c in bf.CASES])
def test_bn_forms(cuda, case):
  assert bf.pool_ties(bf.inputs(case)[0]) == 0  # the oracle and the kernels route a tied maximum alike only by luck
  assert bf.reported_forms(rn.lib(), case) == case['forms']
  threads = torch.get_num_threads()
  torch.set_num_threads(1)  # the float64 references are summed in one order
  try:
    _, errs, bad = bf.run_case(rn.lib(), rn, case, torch.device('cuda'))
  finally:
    torch.set_num_threads(threads)
  for e in errs:
    print('%s %.3e:%g' % e)
  assert not bad, bad
  assert not [e for e in errs if not e[1] < e[2]]
