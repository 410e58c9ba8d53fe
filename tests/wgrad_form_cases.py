"""The filter-gradient kernels (csrc/ra_wgrad.hip) in every launch form their host chooser selects: one table of cases, one runner.

A case names an entry point, its channel counts and the form it is meant to reach with no RA_WGRAD_* variable set.  wgrad has no
plan query, so the name is a label that nothing here asserts: every form passes the same bars, and a chooser that sent a case
to another form would still pass them.  The check on form selection is the cross-build comparison of the digests
(tools/wgrad_digest.py): the forms sum in different orders, so a case that changes form as a rule changes its output bytes.  The
variants below move the cases onto the other forms.  Every case runs at both SHAPES; table calls stack nseg = 3 segments of Bseg = 2 images at unrelated addresses.

  python tests/wgrad_form_cases.py [--lib SO]

runs the whole table in THIS process, under whatever RA_WGRAD_* variables it was started with (the library reads them once per
process), and prints one line per case and shape:  name  sha256 of the output bytes (dw and db, or gw and gb)  err:bar ...
where each err is max |out - ref| / max |ref| against _wgrad_ref in float64 and bar is the project's bar for it.  Inputs come
from a seeded NumPy generator on the host, so two builds of the library see the same bytes and, every kernel summing in a fixed
order, must print the same digests (tools/wgrad_digest.py).  tests/test_wgrad_forms_gpu.py starts this runner once per variant."""
import ctypes as C
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(ROOT, 'rec-attend-public_amd') not in sys.path:
  sys.path.insert(0, os.path.join(ROOT, 'rec-attend-public_amd'))

# (B, H, W) of x.  The first is ragged on both axes against the 8 x 32 tile and spans 2 x 2 tiles over two images: 8 tiles, so
# three workgroups (RA_WGRAD_WGS=3) make 3, 3 and 2 visits; the second is exactly one tile.
SHAPES = [(2, 9, 33), (1, 8, 32)]
NSEG, BSEG = 3, 2

# the environment of each variant; A is what the rest of the suite runs under
VARIANTS = {
    'A': {},
    'B': {'RA_WGRAD_WGS': '3'},                          # several tiles per workgroup: the persistent walk, prefetch, double buffer
    'C': {'RA_WGRAD_WGS': '3', 'RA_WGRAD8': '0'},        # the 16-block form (wgrad_small_kernel) instead of the DMA forms
    'D': {'RA_WGRAD_WGS': '3', 'RA_WGRAD_SMALL': '0'},   # the generic kernel for the 8-output-channel layers too
    'E': {'RA_WGRAD_WGS': '3', 'RA_WGRAD_PRE': '0'},     # no register prefetch of the next tile
    'F': {'RA_WGRAD_WGS': '3', 'RA_WGRAD_PACK': '0'},    # channel rows for every Cin
}

F32_BAR = 2e-5        # test_wgrad_ragged_vs_float64
BF16_BARS = (2e-5, 1e-2)  # test_conv3x3_wgrad_bf16_operands: the oracle on bf16-rounded operands, then on the unrounded ones
STORE_BAR = 2e-5      # test_wgrad8_bf16_storage_vs_float64: the oracle on the same bf16 values

# chan_map of the accumulate cases: packed kernel channel -> filter row, -1 = a padding channel; cin_w rows in the filter
MAPS = {
    8: ([0, 1, 2, -1, 3, 4, -1, -1], 5),
    16: ([0, 1, 2, 3, 4, 5, 6, -1, 7, 8, 9, 10, 11, 12, -1, -1], 13),
}


def _case(entry, cin, cout, form, ups=0, fmt=0, acc=None, table=False):
  """acc: None = dw / db written; ('cut', tr) = no chan_map and cin_w = Cin - 1; ('map', tr) = MAPS[Cin]"""
  name = '%s-%dx%d' % (entry, cin, cout) + ('-ups' if ups else '') + ('-fmt%d' % fmt if fmt else '') + (
      '-%s%s' % (acc[0], '-tr' if acc[1] else '') if acc else '') + ('-table' if table else '')
  return dict(name=name, entry=entry, cin=cin, cout=cout, ups=ups, fmt=fmt, acc=acc, table=table, form=form)


CASES = [
    # float32, ra_conv3x3_wgrad_f32
    _case('f32', 4, 8, 'wgrad8<4>'),
    _case('f32', 8, 8, 'wgrad8<8>'),
    _case('f32', 4, 16, 'generic NT1 PACK4 PRE'),
    _case('f32', 8, 16, 'generic NT1 PACK8 PRE'),
    _case('f32', 4, 32, 'generic NT2 PACK4 PRE'),
    _case('f32', 16, 32, 'generic NT2 PACK0 PRE'),
    _case('f32', 12, 8, 'generic NT1 PACK0 PRE, one partial chunk'),
    _case('f32', 20, 16, 'generic NT1 PACK0 PRE, second chunk with 4 channels'),
    _case('f32', 16, 64, 'generic NT4'),
    _case('f32', 32, 128, 'generic NT4, two slices x two chunks'),
    _case('f32', 8, 2, 'generic NT1 PACK8, scalar dU path, PRE off'),
    _case('f32', 16, 9, 'generic NT1 PACK0, scalar dU path, PRE off'),
    _case('f32', 8, 8, 'generic NT1 PACK8 PRE, upsampled', ups=1),
    _case('f32', 16, 16, 'generic NT1 PACK0 PRE, upsampled', ups=1),
    # bf16 operands, ra_conv3x3_wgrad_bf16ops_f32
    _case('bf16ops', 4, 8, 'generic BF16 NT1 PACK4 PRE'),
    _case('bf16ops', 8, 16, 'generic BF16 NT1 PACK8 PRE'),
    _case('bf16ops', 16, 32, 'generic BF16 NT2 PACK0 PRE'),
    _case('bf16ops', 32, 16, 'generic BF16 NT1 PACK0 PRE, upsampled, two chunks', ups=1),
    _case('bf16ops', 64, 64, 'generic BF16 NT4, four chunks'),
    # bf16 storage, ra_conv3x3_wgrad_acc_bf16_f32 (fmt bit 0: x stored as bf16, bit 1: dU)
    _case('bf16', 8, 8, 'wgrad8b<8>', fmt=3, acc=('cut', 0)),
    _case('bf16', 4, 8, 'wgrad8b<4>', fmt=2, acc=('cut', 0)),
    _case('bf16', 8, 16, 'generic BF16 NT1 PACK8 PRE', fmt=3, acc=('map', 1)),
    _case('bf16', 16, 32, 'generic BF16 NT2 PACK0 PRE', fmt=1, acc=('map', 0)),
    _case('bf16', 16, 32, 'generic BF16 NT2 PACK0 PRE', fmt=2, acc=('cut', 1)),
    # the accumulate forms of the float32 and bf16-operand entries, onto a non-zero gw / gb
    _case('f32', 4, 8, 'wgrad8<4>', acc=('cut', 0)),
    _case('f32', 8, 16, 'generic NT1 PACK8 PRE', acc=('map', 0)),
    _case('f32', 16, 32, 'generic NT2 PACK0 PRE', acc=('map', 1)),
    _case('bf16ops', 16, 32, 'generic BF16 NT2 PACK0 PRE', acc=('map', 1)),
    # the stacked step's pointer-table call, ra_conv3x3_wgrad_multi_acc_f32
    _case('f32', 4, 8, 'wgrad8<4>', acc=('cut', 0), table=True),
    _case('f32', 8, 8, 'wgrad8<8>', acc=('map', 0), table=True),
    _case('bf16', 8, 8, 'wgrad8b<8>', fmt=3, acc=('map', 1), table=True),
    _case('f32', 16, 32, 'generic NT2 PACK0 PRE', acc=('map', 0), table=True),
]


def _wgrad_ref(x, du):
  """dW[ky,kx,ci,co] = sum over pixels of x[.. + tap, ci] * du[.., co] (SAME padding), db = sum du, in float64 on the tensors' device."""
  xi = torch.nn.functional.pad(x.double(), (0, 0, 1, 1, 1, 1))
  B, H, W, Co = du.shape
  d = du.double()
  dw = torch.stack([torch.stack([torch.einsum('bhwc,bhwd->cd', xi[:, ky:ky + H, kx:kx + W], d) for kx in range(3)]) for ky in range(3)])
  return dw, d.sum(dim=(0, 1, 2))


def _rel(a, b):
  return float((a.double() - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _bf16(t):
  return t.bfloat16().float()


def _reference(case, x, du, g0w, g0b, cmap, cin_w):
  """The expected output of a case for host operands x, du (float32 tensors): dw / db, or g0 + the sums in the reference layout."""
  if case['ups']:  # the conv that ran saw x zero-stuffed at the odd positions (a stride-2 transposed conv)
    z = torch.zeros((x.shape[0], 2 * x.shape[1], 2 * x.shape[2], x.shape[3]))
    z[:, 1::2, 1::2] = x
    x = z
  dw, db = _wgrad_ref(x, du)
  if not case['acc']:
    return dw, db
  rows = cmap if cmap is not None else [ci if ci < cin_w else -1 for ci in range(case['cin'])]
  gw = g0w.double().clone()
  for ci, j in enumerate(rows):
    if j < 0:
      continue
    if case['acc'][1]:  # [3,3,Cout,cin_w], taps flipped
      gw[:, :, :, j] += dw[:, :, ci, :].flip(0, 1)
    else:
      gw[:, :, j, :] += dw[:, :, ci, :]
  return gw, g0b.double() + db


def run_case(lib, rn, case, shape, dev):
  """Launches one case at one shape; returns (sha256 of the output bytes, [(err, bar), ...])."""
  B, Hs, Ws = shape
  cin, cout, ups, fmt, table = case['cin'], case['cout'], case['ups'], case['fmt'], case['table']
  H, W = Hs * (1 + ups), Ws * (1 + ups)
  nseg = NSEG if table else 1
  Bs = BSEG if table else B
  rng = np.random.RandomState(1000 * cin + 10 * cout + H + 7 * fmt + (3 if table else 0))
  x = torch.from_numpy(rng.randn(nseg * Bs, Hs, Ws, cin).astype(np.float32))
  du = torch.from_numpy(rng.randn(nseg * Bs, H, W, cout).astype(np.float32))
  xbf, ubf = bool(fmt & 1), bool(fmt & 2)
  keep = []  # junk between the segments keeps them at unrelated addresses

  def put(t, bf):
    segs = []
    for s in range(nseg):
      d = t[s * Bs:(s + 1) * Bs].to(dev)
      segs.append(d.bfloat16() if bf else d)
      keep.append(torch.full((1000 + 77 * s,), float('nan'), device=dev))
    return segs
  xs, us = put(x, xbf), put(du, ubf)
  nws = lib.ra_conv3x3_wgrad_workspace_floats(cin, cout, nseg * Bs, H, W)
  ws = torch.full((nws,), float('nan'), device=dev)
  acc = case['acc']
  cmap = cin_w = None
  if acc:
    cmap, cin_w = MAPS[cin] if acc[0] == 'map' else (None, cin - 1)
    shape_w = (3, 3, cout, cin_w) if acc[1] else (3, 3, cin_w, cout)
    g0w, g0b = torch.from_numpy(rng.randn(*shape_w).astype(np.float32)), torch.from_numpy(rng.randn(cout).astype(np.float32))
    ow, ob = g0w.to(dev), g0b.to(dev)
    cm = torch.tensor(cmap, dtype=torch.int32, device=dev) if cmap is not None else None
    tail = (rn.ptr(cm) if cm is not None else None, cin_w, acc[1], rn.ptr(ow), rn.ptr(ob))
  else:
    g0w = g0b = None
    ow, ob = torch.full((3, 3, cin, cout), 7.0, device=dev), torch.full((cout,), 7.0, device=dev)
  head = (cin, Bs, Hs, Ws, ups)
  entry = case['entry']
  if table:
    tab = torch.zeros(128, dtype=torch.int64, device=dev)
    for off, ts in ((0, xs), (64, us)):
      host = (C.c_void_p * nseg)(*[t.data_ptr() for t in ts])
      rn.check(lib.ra_ptr_table(host, nseg, tab.data_ptr() + 8 * off, rn.stream_ptr()), 'ra_ptr_table')
    flags = {'f32': 0, 'bf16ops': 1, 'bf16': 1 | (fmt << 1)}[entry]
    rn.check(lib.ra_conv3x3_wgrad_multi_acc_f32(tab.data_ptr(), tab.data_ptr() + 8 * 64, nseg, *head, cout, rn.ptr(ws), nws, *tail, flags,
                                                rn.stream_ptr()), case['name'])
  elif entry == 'bf16':
    rn.check(lib.ra_conv3x3_wgrad_acc_bf16_f32(rn.ptr(xs[0]), *head, rn.ptr(us[0]), cout, rn.ptr(ws), nws, *tail, fmt, rn.stream_ptr()),
             case['name'])
  elif acc:
    fn = lib.ra_conv3x3_wgrad_acc_bf16ops_f32 if entry == 'bf16ops' else lib.ra_conv3x3_wgrad_acc_f32
    rn.check(fn(rn.ptr(xs[0]), *head, rn.ptr(us[0]), cout, rn.ptr(ws), nws, *tail, rn.stream_ptr()), case['name'])
  else:
    fn = lib.ra_conv3x3_wgrad_bf16ops_f32 if entry == 'bf16ops' else lib.ra_conv3x3_wgrad_f32
    rn.check(fn(rn.ptr(xs[0]), *head, rn.ptr(us[0]), cout, rn.ptr(ws), nws, rn.ptr(ow), rn.ptr(ob), rn.stream_ptr()), case['name'])
  torch.cuda.synchronize()
  ow, ob = ow.cpu(), ob.cpu()
  sha = hashlib.sha256(ow.numpy().tobytes() + ob.numpy().tobytes()).hexdigest()
  if entry == 'f32':
    refs = [((x, du), F32_BAR)]
  elif entry == 'bf16ops':
    refs = [((_bf16(x), _bf16(du)), BF16_BARS[0]), ((x, du), BF16_BARS[1])]
  else:
    refs = [((_bf16(x), _bf16(du)), STORE_BAR)]
  errs = []
  for (xa, da), bar in refs:
    rw, rb = _reference(case, xa, da, g0w, g0b, cmap, cin_w)
    errs += [(_rel(ow, rw), bar), (_rel(ob, rb), bar)]
  del keep
  return sha, errs


def parse_line(line):
  """A runner line -> (name, sha256, [(err, bar), ...]), or None for any other line."""
  f = line.split()
  if len(f) < 3 or f[0] != 'case':
    return None
  return f[1], f[2], [tuple(float(v) for v in p.split(':')) for p in f[3:]]


def main():
  import argparse
  ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
  ap.add_argument('--lib', help='the librecattend.so to run (default: the tree\'s own)')
  args = ap.parse_args()
  import ra_native as rn
  if args.lib:
    rn.LIB_PATH = os.path.abspath(args.lib)
  if not torch.cuda.is_available():
    raise SystemExit('wgrad_form_cases: needs an MI355X')
  torch.set_num_threads(1)  # the float64 references are summed in one order
  dev = torch.device('cuda')
  lib = rn.lib()
  for case in CASES:
    for shape in SHAPES:
      sha, errs = run_case(lib, rn, case, shape, dev)
      print('case %s@%s %s %s' % (case['name'], 'x'.join(map(str, shape)), sha, ' '.join('%.3e:%g' % p for p in errs)), flush=True)


if __name__ == '__main__':
  main()
