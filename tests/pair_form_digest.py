"""The fused-pair kernels (csrc/ra_conv_pair.hip, csrc/ra_conv_pair8.hip) in every launch form, as digests of their output bytes.

  python tests/pair_form_digest.py [--lib SO] [--check]

walks, in THIS process and under whatever RA_PAIR* variables it was started with (the library reads them once per process),
  * conv_form_cases.PAIR_CASES + PAIR_WALK_CASES, on the seeded inputs of test_conv_forms_gpu.py::test_pair_forms
    (test_conv_forms_gpu.pair_case), the cached forms launched as that test launches them;
  * the upsampleA shapes of test_kernels_gpu.py::test_conv_pair's table (the zero-stuffed one-shot staging);
  * one rider case: the cache-filling launch with a constant fill of another buffer riding on it,
and prints one line per case:  case <shape> out:<sha256 of the output bytes> [cache:<sha256>] [rider:<sha256>] [err:<e>:<bar>]
plan <the plan the query reports>.  No pair kernel uses atomics on its results and every sum has a fixed order, so two builds
of the library compute the same thing exactly when tools/pair_digest.py's dumps of them are byte-identical.

VARIANTS moves the cases onto the kernels the default dispatch does not take them to; tests/test_pair_variants_gpu.py starts this
runner once per non-default variant.  --check: each output against the float64 oracle at test_pair_forms' bar, the plan of
every table case against the one it names (default variant only), guard words of the rider; exit status 1 if anything misses.
The last line counts the cases launched.  The cached forms never go through ra_conv_pair_f32, so RA_PAIR_NO8 cannot move them:
under it they are counted and not launched."""
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, 'rec-attend-public_amd'), os.path.join(ROOT, 'oracle')):
  if _p not in sys.path:
    sys.path.insert(0, _p)

# the environment of each variant; 'default' is what the rest of the suite runs under
VARIANTS = {
    'default': {},
    'onepass': {'RA_PAIR_PERSIST': '0'},  # the persistent shapes through the one-shot kernel
    'no8': {'RA_PAIR_NO8': '1'},          # the N-packed shapes through the generic pair, canvas plane included
    'f32b': {'RA_PAIR8_SPLIT': '0'},      # the cached kernel with layer B on the float32 MFMA
}

BAR = 3e-5          # test_pair_forms / test_conv_pair: of the output scale
RIDER_FLOATS = 3 * 256 * 4 * 7  # a multiple of 4 floats that no grid divides evenly (test_first_layer_cache_vs_plain_pair)
RIDER_SHAPE = (3, 50, 70, 4, 8, 8, 0, 2, 1, 1)


def cases():
  """(shape, expected plan or None, rider) of every case; shape = (B, Hs, Ws, Cin, CoutA, CoutB, upsA, poolB, plane, cache_form)."""
  import conv_form_cases as cf
  import test_kernels_gpu as tk
  out = [(s, p, False) for s, p in cf.PAIR_CASES] + [(c[0], c[1], False) for c in cf.PAIR_WALK_CASES]
  out += [((B, H, W, Ci, Ca, Cb, 1, pool, 0, 0), None, False) for B, H, W, Ci, Ca, Cb, pool, ups in tk.PAIR_CASES if ups]
  return out + [(RIDER_SHAPE, None, True)]


def n_cache_form():
  return sum(1 for s, _, _ in cases() if s[9])


def sha(t):
  return hashlib.sha256(t.detach().cpu().numpy().tobytes()).hexdigest()


def run_case(shape, rider, check, cuda):
  """Launches one case; returns (fields of its line, list of what missed)."""
  import ra_ops as ops
  import test_conv_forms_gpu as tf
  B, Hs, Ws, Ci, Ca, Cb, ups, pool, has_plane, cache_form = shape
  x, xr, plane, (wpA, scA, shA), (wpB, scB, shB), ref_of = tf.pair_case(shape, cuda)
  d = lambda a: tf.dev(a, cuda)
  what = 'pair %r' % (shape,)
  out = tf.Guarded((B, Hs * (1 + ups) // pool, Ws * (1 + ups) // pool, Cb), cuda)
  fields, bad, ref_in = [], [], xr
  if cache_form == 0:
    ops.conv_pair(d(x), wpA, scA, shA, Ca, wpB, scB, shB, Cb, poolB=pool, upsampleA=bool(ups), out=out.view, plane=d(plane) if has_plane else None,
                  plane_chan=3 if has_plane else -1)
  else:
    zero = torch.zeros((B, Hs, Ws), device=cuda)
    cache = ops.first_cache_alloc(B, Hs, Ws, cuda)
    buf = torch.full((RIDER_FLOATS + 8,), 7.0, dtype=torch.float32, device=cuda) if rider else None
    first = out.view if cache_form == 1 else torch.empty_like(out.view)
    ops.conv_pair_fill_cache(d(x), zero, 3, wpA, scA, shA, wpB, scB, shB, Cb, cache, first, fill=buf[4:4 + RIDER_FLOATS] if rider else None,
                             fill_value=0.25)
    if cache_form == 1:
      ref_in = xr.copy()
      ref_in[..., 3] = 0.0
    else:
      ops.conv_pair_cached(cache, d(plane), 3, wpA, scA, shA, wpB, scB, shB, Cb, out.view)
    fields.append('cache:' + sha(cache))
    if rider:
      fields.append('rider:' + sha(buf))
      got = buf.cpu().numpy()
      if not ((got[:4] == 7.0).all() and (got[4 + RIDER_FLOATS:] == 7.0).all() and (got[4:4 + RIDER_FLOATS] == 0.25).all()):
        bad.append('the rider fill wrote outside its buffer or left a hole')
  y = out.result(what)  # guard words intact, every element written
  fields.insert(0, 'out:' + hashlib.sha256(y.tobytes()).hexdigest())
  if check:
    ref = ref_of(ref_in)
    e = np.abs(y.astype(np.float64) - ref).max() / max(1e-6, np.abs(ref).max())
    fields.append('err:%.3e:%g' % (e, BAR))
    if not e < BAR:
      bad.append('%.3g of the output scale >= %g' % (e, BAR))
  return fields, bad


def parse_line(line):
  """A runner line -> (shape string, {field: value}, plan), or None for any other line."""
  f = line.split()
  if len(f) < 4 or f[0] != 'case' or 'plan' not in f:
    return None
  i = f.index('plan')
  return f[1], dict(q.split(':', 1) for q in f[2:i]), ' '.join(f[i + 1:])


def main():
  import argparse
  ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
  ap.add_argument('--lib', help='the librecattend.so to run (default: the tree\'s own)')
  ap.add_argument('--check', action='store_true', help='compare with the float64 oracle and the named plans; status 1 on a miss')
  args = ap.parse_args()
  import ra_native as rn
  if args.lib:
    rn.LIB_PATH = os.path.abspath(args.lib)
  if not torch.cuda.is_available():
    raise SystemExit('pair_form_digest: needs an MI355X')
  import conv_form_cases as cf
  cuda = torch.device('cuda')
  no8 = bool(os.environ.get('RA_PAIR_NO8'))
  default = not any(k.startswith('RA_PAIR') for k in os.environ)
  ran, broken, all_cases = 0, 0, cases()
  for shape, expected, rider in all_cases:
    name = 'x'.join(map(str, shape)) + ('+rider' if rider else '')
    if no8 and shape[9]:
      print('skipped %s: a cached form, which RA_PAIR_NO8 does not move' % name, flush=True)
      continue
    plan = cf.plan_str(cf.pair_plan(shape))
    fields, bad = run_case(shape, rider, args.check, cuda)
    ran += 1
    print('case %s %s plan %s' % (name, ' '.join(fields), plan), flush=True)
    if args.check and default and expected is not None and plan != expected:
      bad.append('the dispatch no longer takes this case to its form %s' % expected)
    for b in bad if args.check else []:
      print('BROKEN %s: %s' % (name, b), flush=True)
      broken += 1
  floor = len(all_cases) - n_cache_form()
  print('ran %d of %d cases (%d cached forms)' % (ran, len(all_cases), n_cache_form()), flush=True)
  if args.check and ran < floor:
    print('BROKEN: fewer than %d cases ran' % floor, flush=True)
    broken += 1
  return 1 if broken else 0


if __name__ == '__main__':
  sys.exit(main())
