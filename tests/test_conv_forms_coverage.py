"""Form coverage of tests/test_conv_forms_gpu.py, for the plan queries that need no device: every plan ra_conv3x3_plan (K1, its
bf16-operand, moments and k x k parts) and ra_conv_pair_plan (the pair's geometry, the N-packed kernel) return over the declared
grid of shapes is the plan of a case in tests/conv_form_cases.py.  A dispatch threshold that moves, or a new instantiation,
fails here until a case reaches it.  (The plans that follow the device's CU count are counted by the GPU-marked
test_device_plans_are_covered.)"""
import conv_form_cases as cf


def _k1_rows(kind):
  kw = cf.K1_KINDS[kind]
  bf16, mom, kf = int(kw.get('bf16', 0)), int(kw.get('moments', 0)), kw.get('ksize', 3)
  for ci in cf.K1_CIN:
    for co in cf.K1_COUT:
      for pool in (1, 2):
        for ups in (0, 1):
          for B in cf.COVER_B:
            for H in cf.COVER_HW:
              for W in cf.COVER_HW:
                # C0, C1, B, Hs, Ws, upsample, KF, Cout, pool, has_plane, bf16_operands, moments, store_flags
                yield (ci, 0, B, H, W, ups, kf, co, pool, 0, bf16, mom, 0)


def test_every_k1_plan_is_covered():
  cases = {(kind, plan) for kind, _, plan in cf.K1_CASES + cf.K1_EXTRA_CASES}
  reached, uncovered = 0, []
  for kind in cf.K1_KINDS:
    plans = cf.distinct_plans('conv3x3', _k1_rows(kind))
    reached += len(plans)
    uncovered += sorted((kind, p) for p in plans if (kind, p) not in cases)
  print('K1: %d distinct (entry, plan) over the grid, %d uncovered' % (reached, len(uncovered)))
  assert reached >= 400  # the grid really spans the dispatch (five geometries x store forms x (NC, WN) x CK x the parts)
  assert not uncovered, uncovered


def test_every_case_reaches_its_plan_without_a_device():
  """The K1 tables name the plan the query returns here as on the GPU: no device fact enters a K1 choice."""
  for kind, shape, plan in cf.K1_CASES + cf.K1_EXTRA_CASES:
    assert cf.plan_str(cf.k1_plan(kind, shape)) == plan, (kind, shape)


def pair_rows():
  for B in cf.COVER_B:
    for H in cf.COVER_HW:
      for W in cf.COVER_HW:
        for ci, ca, cb in cf.PAIR_CHANNELS:
          for ups in (0, 1):
            if B * H * W * (4 if ups else 1) > 1 << 24:
              continue  # (a 2 GiB tensor at 32 channels; the thresholds are far below)
            for pool in (1, 2):
              for plane in (0, 1):
                yield (ci, B, H, W, ups, ca, cb, pool, plane, 0)  # Cin, B, Hs, Ws, upsampleA, CoutA, CoutB, poolB, has_plane, cache_form
        for cb in (1, 5, 8):
          for cache_form in (1, 2):
            yield (4, B, H, W, 0, 8, cb, 2, 1, cache_form)


def test_every_pair_geometry_is_covered():
  """Whether the persistent kernel runs is the device's to say (its occupancy): that bit is left out on both sides here."""
  cases = {cf.strip_form(plan, ('persist',)) for _, plan in cf.PAIR_CASES} | {cf.strip_form(c[1], ('persist',)) for c in cf.PAIR_WALK_CASES}
  plans = cf.distinct_plans('conv_pair', pair_rows(), drop_form=('persist',))
  uncovered = sorted(plans - cases)
  print('pair: %d distinct geometries over the grid, %d uncovered' % (len(plans), len(uncovered)))
  assert len(plans) >= 80 and not uncovered, uncovered
