"""The controller kernels (csrc/ra_ctrl.hip, csrc/ra_ctrl_split.hip) in every form and exchange variant: one table of cases, one runner.

RA_CTRL_XCD is read once per process, so two variants of the exchange code are reached by no test of tests/test_kernels_gpu.py:
RA_CTRL_XCD=0 (the agent-scope exchange for the per-image form at B <= 8 and for the group-shared form with an XCD offset
given) and RA_CTRL_XCD=2 (the XCD-local per-image form with two teams on an XCD, B = 11).

  python tests/ctrl_form_cases.py [--lib SO]

runs the whole table in THIS process, under whatever RA_CTRL_XCD it was started with, and prints one line per case and form:
  case NAME  sha256 of the h_last | ctrl_out | gmaps | attn bytes of its three launches  status=WORD  err:bar ...
Every case makes three launches on ONE workspace (generation tags and role tickets only ever count up), each on other
features; an err is the largest over the three against ora._controller / ora._decode_ctrl in float64, and the bars are the table
of errors() below, which tests/test_kernels_gpu.py (_CtrlCase.check) asserts too; entries that must be exact (fixed gammas, the record's zero tail) are
printed as their largest deviation with the bar EXACT.  Inputs come from seeded NumPy generators on the host, no kernel here
uses float atomics and every sum has a fixed order, so two builds of the library must print the same digests
(tools/ctrl_digest.py).  tests/test_ctrl_forms_gpu.py starts this runner once per variant."""
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
    'xcd0': {'RA_CTRL_XCD': '0'},   # agent-scope exchange everywhere
    'xcd2': {'RA_CTRL_XCD': '2'},   # the XCD-local per-image form beyond 8 images too: two teams on an XCD at B = 11
}

# G = 16, and G = 49: padded logits (gs = 4) and a ragged last slice
DESCS = [('cvppp', 128, 128, {}), ('cvppp', 224, 224, {'squash_ctrl_params': True})]
BATCHES = [1, 5, 8, 11]
# (label, entry, xcd_offset): the one-workgroup kernel, 16 workgroups per image, 16 per group of images
FORMS = [('one', 'one', None), ('split', 'split', None), ('batch-agent', 'batch', -1), ('batch-xcd0', 'batch', 0), ('batch-xcd5', 'batch', 5)]
EXACT = 1e-30  # the bar printed for entries that must be exact: their deviation is 0.0 or the case fails


def case_names():
  return ['%s-%dx%d-B%d-%s' % (arch, H, W, B, form[0]) for arch, H, W, _ in DESCS for B in BATCHES for form in FORMS]


def _relerr(a, b):
  return float(np.abs(a - b).max() / max(1e-6, np.abs(b).max()))


def errors(d, H, W, ref, h_last, ctrl_out, gmaps, a):
  """The checks of one controller launch, as [(what, err, bar), ...]: h_last, ctrl_out, the glimpse maps and the WHOLE attention
  record a [B, 16] (entries 0..12, the zero tail 13..15) against ref = (h, co, gm) of ora._controller + (cn, ls, ctr, size, lv)
  of ora._decode_ctrl in float64; the launch passes where every err < bar.  The one table of the controller's bars:
  tests/test_kernels_gpu.py (_CtrlCase.check) asserts it and the runner below prints it."""
  h, co, gm, cn, ls, ctr, size, lv = ref
  amax = lambda x, y: float(np.abs(x - y).max())
  out = [('h_last', _relerr(h_last, h), 5e-5), ('ctrl_out', amax(ctrl_out, co), 5e-5), ('gmaps', amax(gmaps, gm), 1e-5),
         ('centre', amax(a[:, 0:2], ctr), 1e-3 * max(H, W) / 100), ('size', _relerr(a[:, 2:4], size), 1e-4),
         ('log-variance', amax(a[:, 4:6], lv), 1e-4), ('cn', amax(a[:, 9:11], cn), 1e-4), ('ls', amax(a[:, 11:13], ls), 1e-4)]
  if d['fixed_gamma']:
    out += [('gamma 6 == 1', amax(a[:, 6], 1.0), EXACT), ('gamma 8 == 2', amax(a[:, 8], 2.0), EXACT)]
  else:
    out += [('gamma 6', _relerr(a[:, 6], np.exp(co[:, 6])), 1e-4), ('gamma 8', amax(a[:, 8], co[:, 8]), 1e-4)]
  return out + [('gamma 7', _relerr(a[:, 7], np.exp(co[:, 7])), 1e-4), ('zero tail', amax(a[:, 13:16], 0.0), EXACT)]


def run(dev):
  """Yields (name, sha256, status word, [(err, bar), ...]) for every case and form."""
  import ra_ops as ops
  import ra_oracle as ora
  for arch, H, W, flags in DESCS:
    opt = ora.make_opt(arch, H, W, 2, **flags)
    d, P = ora.derive(opt), ora.random_params(opt, 4)
    P64 = {k: v.astype(np.float64) for k, v in P.items()}
    Cf = d['ccnn_channels'][-1]
    desc = ops.make_ctrl_desc(d['G'], Cf, d['hid'], d['iters'], d['n_gmlp'], d['n_cmlp'], opt['ctrl_mlp_dim'], H, W, 48, 48, d['squash'],
                              d['fixed_var'], d['dynamic_var'], d['fixed_gamma'])
    lstm = {k[len('ctrl_lstm_'):]: v for k, v in P.items() if k.startswith('ctrl_lstm_')}
    gmw = [(P['glimpse_mlp_w_%d' % i], P['glimpse_mlp_b_%d' % i]) for i in range(d['n_gmlp'])]
    cmw = [(P['ctrl_mlp_w_%d' % i], P['ctrl_mlp_b_%d' % i]) for i in range(d['n_cmlp'])]
    wp_one = torch.from_numpy(ops.pack_ctrl_weights(desc, lstm, gmw, cmw)).to(dev)
    wp_split = torch.from_numpy(ops.pack_ctrl_split_weights(desc, lstm, gmw, cmw)).to(dev)
    for B in BATCHES:
      feats, refs = [], []  # the three launches' features and float64 references, shared by the forms
      for rep in range(3):
        f = np.maximum(np.random.RandomState(100 * B + rep).randn(B, d['G'], Cf), 0).astype(np.float32)
        h, co, gm = ora._controller(d, P64, f.astype(np.float64), np.dtype(np.float64))
        feats.append(f)
        refs.append((h, co, gm) + tuple(ora._decode_ctrl(d, co, np.dtype(np.float64))))
      for label, entry, xcd_off in FORMS:
        if entry == 'split':
          ws, status = ops.ctrl_split_workspace(desc, B, dev)
        elif entry == 'batch':
          ws, status = ops.ctrl_batch_workspace(desc, B, dev)
        else:
          status = torch.zeros(1, dtype=torch.int32, device=dev)
        sha, worst = hashlib.sha256(), None
        for f, ref in zip(feats, refs):
          out = [torch.full(s, 7.0, dtype=torch.float32, device=dev) for s in ((B, d['hid']), (B, 9), (B, d['iters'], d['G']), (B, 16))]
          fd = torch.from_numpy(f).to(dev)
          if entry == 'split':
            ops.controller_split(desc, fd, wp_split, *out, ws, status)
          elif entry == 'batch':
            ops.controller_batch(desc, fd, wp_split, *out, ws, status, xcd_offset=xcd_off)
          else:
            ops.controller(desc, fd, wp_one, *out)
          torch.cuda.synchronize()
          out = [t.cpu().numpy() for t in out]
          for t in out:
            sha.update(t.tobytes())
          errs = [(e, bar) for _, e, bar in errors(d, H, W, ref, *out)]
          worst = errs if worst is None else [(max(e, w), bar) for (e, bar), (w, _) in zip(errs, worst)]
        yield '%s-%dx%d-B%d-%s' % (arch, H, W, B, label), sha.hexdigest(), int(status.item()), worst


def parse_line(line):
  """A runner line -> (name, sha256, status word, [(err, bar), ...]), or None for any other line."""
  f = line.split()
  if len(f) < 5 or f[0] != 'case' or not f[3].startswith('status='):
    return None
  return f[1], f[2], int(f[3][len('status='):]), [tuple(float(v) for v in p.split(':')) for p in f[4:]]


def main():
  import argparse
  ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
  ap.add_argument('--lib', help='the librecattend.so to run (default: the tree\'s own)')
  args = ap.parse_args()
  import ra_native as rn
  if args.lib:
    rn.LIB_PATH = os.path.abspath(args.lib)
  if not torch.cuda.is_available():
    raise SystemExit('ctrl_form_cases: needs an MI355X')
  for name, sha, status, errs in run(torch.device('cuda')):
    print('case %s %s status=%d %s' % (name, sha, status, ' '.join('%.3e:%g' % p for p in errs)), flush=True)
    if status != 0:  # a team waited for a peer that never arrived (kSpinLimit): nothing more is launched
      raise SystemExit('ctrl_form_cases: status word %d after %s; stopping' % (status, name))


if __name__ == '__main__':
  main()
