#!/usr/bin/env python
"""The output bytes of the direct attention kernels (csrc/ra_attn_direct.hip, ra_attn_train.hip) as digests: one child process
under its own time limit runs the records of every shape of tests/attn_geometry_cases.py (all_shapes() and ADJOINT_SHAPES)
through each entry point and prints one sha256 per (shape, entry, variant) over the bytes the launches wrote.  These kernels sum
in a fixed order without atomics, so two builds compute the same outputs exactly when their dumps are byte-identical:

  python tools/attn_digest.py --lib OTHER/rec-attend-public_amd/librecattend.so --out a.txt
  python tools/attn_digest.py --out b.txt && cmp a.txt b.txt

--lib: the library to load (default: the one beside the package).  Reads only what the tests read."""
import argparse
import hashlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(lib):
  for p in (os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'rec-attend-public_amd')):
    sys.path.insert(0, p)
  import numpy as np
  import torch
  import ra_native as rn
  if lib:
    rn.LIB_PATH = lib
  if not torch.cuda.is_available():
    raise SystemExit('attn_digest: needs an MI355X')
  import attn_geometry_cases as ag
  import ra_ops as ops
  import test_attn_geometry_gpu as tg
  cuda, B = 'cuda', ag.B_LAUNCH
  dev = lambda a: tg.dev(a, cuda)

  class Digest:
    def __init__(self, sid, entry, variant='-'):
      self.key, self.sha = (sid, entry, variant), hashlib.sha256()

    def take(self, *arrays):
      torch.cuda.synchronize()
      for a in arrays:
        if a is not None:
          self.sha.update(np.ascontiguousarray(a.detach().cpu().numpy() if torch.is_tensor(a) else a).tobytes())

    def done(self):
      print('digest %s %s %s %s' % (self.key + (self.sha.hexdigest(),)), flush=True)

  combos = [(o, f) for f in tg.FLAG_MODES for o in (0, 1)]
  for sid, (H, W, Fh, Fw) in ag.all_shapes().items():
    ref = ag.reference(sid)
    batches = tg._batches(ref)
    for vi, (plane, use_gamma, (chan0, Cp, cchan)) in enumerate(tg.EXTRACT_VARIANTS):
      d = Digest(sid, 'extract_direct', 'v%d' % vi)
      for k, sl in batches:
        img = np.array(ref['img'][sl])
        img[..., cchan] = -50.0 if plane else ref['canvas'][sl]
        patch = torch.full((B, Fh, Fw, Cp), tg.SENT, dtype=torch.float32, device=cuda)
        ops.extract_direct(dev(img), chan0, dev(ref['rec'][sl]), Fh, Fw, Cp, use_gamma, patch,
                           canvas=dev(ref['canvas'][sl]) if plane else None, canvas_chan=cchan if plane else -1)
        d.take(patch)
      d.done()
    if Fw <= 64:
      d, rng = Digest(sid, 'extract_conv0'), np.random.RandomState(len(sid))
      for k, sl in batches:   # the arguments of test_extract_conv0
        plane, use_gamma, cout, chan0 = k % 2, (k // 2) % 2, (8, 12, 16)[k % 3], 4 * ((k // 4) % 2)
        img = np.array(ref['img'][sl])
        img[..., chan0 + 3] = -50.0 if plane else ref['canvas'][sl]
        w0 = (rng.randn(3, 3, 4, cout) * 0.3).astype(np.float32)
        cp = ops.cout_padded(cout)
        sc, sh = np.ones(cp, np.float32), np.zeros(cp, np.float32)
        sc[:cout], sh[:cout] = rng.uniform(0.5, 1.5, cout), rng.randn(cout) * 0.2
        patch = torch.full((B, Fh, Fw, 4), tg.SENT, dtype=torch.float32, device=cuda)
        y0 = torch.full((B, Fh, Fw, cout), tg.SENT, dtype=torch.float32, device=cuda)
        ops.extract_conv0(dev(img), chan0, dev(ref['rec'][sl]), Fh, Fw, use_gamma, patch, dev(w0), dev(sc), dev(sh), cout, True, y0,
                          canvas=dev(ref['canvas'][sl]) if plane else None, canvas_chan=chan0 + 3 if plane else -1)
        d.take(patch, y0)
      d.done()
    for variant in ag.paste_variants(sid) if sid in ag.PASTE_CASES else ():   # the case table's extract-only shape has none
      if ag.PASTE_VARIANTS[variant]['mode'] == 'box':
        d = Digest(sid, 'attn_box_direct', variant)
        for k, sl in batches:
          ybuf = tg.YBuffer(cuda, H, W, tg.SENT, odd=variant == 'box_stride')
          ops.attn_box_direct(dev(ref['rec'][sl]), H, W, Fh, Fw, ag.BETA, ybuf.ptr, ybuf.stride)
          d.take(ybuf.buf)
        d.done()
        continue
      d = Digest(sid, 'paste_direct', variant)
      for k, sl in batches:
        for overwrite, flags in combos:
          y, cv, _, _ = tg._paste_launch(cuda, sid, ref, sl, variant, overwrite, flags)
          d.take(y, cv)
      d.done()
      if ag.PASTE_VARIANTS[variant]['has_canvas']:
        d, rng = Digest(sid, 'paste_score_direct', variant), np.random.RandomState(11)
        for k, sl in batches:   # the arguments of test_paste_score_direct
          overwrite, flags = combos[k % 6]
          K0, K1, s_stride = (300, 70, 37)[k % 3], (0, 33)[k % 2], (1, 3)[(k // 2) % 2]
          h, w, bias = rng.randn(B, K0).astype(np.float32), (rng.randn(K0 + K1) / 8).astype(np.float32), rng.randn(1).astype(np.float32)
          core = rng.randn(B, K1).astype(np.float32) if K1 else None
          s_buf = torch.full((B * s_stride,), tg.SENT, dtype=torch.float32, device=cuda)
          score = (dev(h), None if core is None else dev(core), dev(w), dev(bias), s_buf, s_stride)
          y, cv, _, _ = tg._paste_launch(cuda, sid, ref, sl, variant, overwrite, flags, score=score)
          d.take(y, cv, s_buf)
        d.done()
  for sid in ag.ADJOINT_SHAPES:
    case = ag.adjoint_case(sid)
    H, W, Fh, Fw = case['dims']
    n = case['rec'].shape[0]
    y_any = (1.0 / (1.0 + np.exp(-case['wB']))).astype(np.float32)   # a plane in (0, 1) for the forward value the adjoint reads
    for mode, name in ((ops.RESAMPLE_READ, 'read'), (ops.RESAMPLE_WRITE, 'write'), (ops.RESAMPLE_BOX, 'box')):
      d = Digest(sid, 'resample_bwd', name)
      for lo in range(0, n, B):
        sl = slice(lo, lo + B)
        rec = dev(case['rec'][sl])
        if mode == ops.RESAMPLE_READ:
          E = torch.full((B, Fh, Fw, 4), tg.SENT, dtype=torch.float32, device=cuda)
          out = ops.resample_bwd(mode, rec, H, W, Fh, Fw, X=dev(case['x'][sl]), Q=dev(case['wE'][sl]), E=E, scale=rec[:, 6])
        elif mode == ops.RESAMPLE_WRITE:
          E = torch.full((B, Fh, Fw, 1), tg.SENT, dtype=torch.float32, device=cuda)
          out = ops.resample_bwd(mode, rec, H, W, Fh, Fw, dY=dev(case['wY'][sl]), Y=dev(y_any[sl]), Q=dev(case['P'][sl][..., None]), E=E)
        else:
          E = None
          out = ops.resample_bwd(mode, rec, H, W, Fh, Fw, dY=dev(case['wB'][sl]), Y=dev(y_any[sl]), div=rec[:, 7])
        d.take(out, E)
      d.done()


def main():
  ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
  ap.add_argument('--lib', help='the librecattend.so to run (default: the one beside the package)')
  ap.add_argument('--out')
  ap.add_argument('--timeout', type=int, default=300, help='seconds for the child')
  ap.add_argument('--child', action='store_true', help='run the cases in this process (what the driver starts)')
  args = ap.parse_args()
  lib = os.path.abspath(args.lib) if args.lib else None
  if args.child:
    return child(lib)
  if not args.out:
    ap.error('--out is required')
  cmd = ['timeout', '-k', '10', str(args.timeout), sys.executable, os.path.abspath(__file__), '--child']
  r = subprocess.run(cmd + (['--lib', lib] if lib else []), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
  lines = [t[len('digest '):] for t in r.stdout.splitlines() if t.startswith('digest ')]
  if r.returncode != 0 or not lines:
    sys.stdout.write(r.stdout)
    print('attn_digest: the child ended with status %d' % r.returncode)
    return r.returncode if r.returncode > 0 else 1
  with open(args.out, 'w') as out:
    out.write('\n'.join(lines) + '\n')
  print('%d digests, sha256 of the file %s' % (len(lines), hashlib.sha256(('\n'.join(lines) + '\n').encode()).hexdigest()))
  return 0


if __name__ == '__main__':
  sys.exit(main())
