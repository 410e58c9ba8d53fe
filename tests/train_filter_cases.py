"""What the tests of training with filter sizes 1, 5 and 7 share (test_train_filter_sizes.py, test_train_filter_sizes_gpu.py):
the differentiable float64 reference of the stride-2 transposed conv, the float64 filter gradient for a KF x KF window, and
the inputs of the whole-step comparison."""
import numpy as np
import torch
import torch.nn.functional as F

import ra_oracle as ora
import ra_oracle_torch as ort

SIZES = (1, 5, 7)


def pad_lo(kf):
  """TF's SAME padding in front of a stride-2 conv over an even-sized image: max(KF - 2, 0) // 2."""
  return max(kf - 2, 0) // 2


def deconv_ref(x, w, b, stride):
  """ra_oracle_torch.deconv_same for every odd filter size: conv2d_transpose(x, w [f,f,out,in], SAME), NHWC.  Stride 2 is
  conv_transpose2d(stride=2, padding=0)[pt:pt + 2H, pl:pl + 2W] with pt = pl = max(f - 2, 0) // 2, zero-filled where the
  full output is short (f = 1); ra_oracle_torch's own crops at 0, which is right for f = 3 alone."""
  if ort._rounds_operands():
    x, w = ort._RoundOperand.apply(x), ort._RoundOperand.apply(w)
  f = w.shape[0]
  wt = w.permute(3, 2, 0, 1)  # [in, out, kh, kw]
  xi = x.permute(0, 3, 1, 2)
  if stride == 1:
    y = F.conv_transpose2d(xi, wt, stride=1, padding=f // 2)
  else:
    assert stride == 2
    n_h, n_w = 2 * x.shape[1], 2 * x.shape[2]
    p = pad_lo(f)
    full = F.conv_transpose2d(xi, wt, stride=2, padding=0)[:, :, p:p + n_h, p:p + n_w]
    y = F.pad(full, (0, n_w - full.shape[3], 0, n_h - full.shape[2]))
  y = y.permute(0, 2, 3, 1) + b
  return ort._RoundGradient.apply(y) if ort._rounds_operands() else y


def wgrad_ref(x, du, kf):
  """wgrad_form_cases._wgrad_ref for a KF x KF window: dW[ky,kx,ci,co] = sum over pixels of x[.. + tap - KF // 2, ci] *
  du[.., co] (SAME padding), db = sum du, in float64 on the tensors' device."""
  p = kf // 2
  xi = F.pad(x.double(), (0, 0, p, p, p, p))
  B, H, W, Co = du.shape
  d = du.double()
  dw = torch.stack([torch.stack([torch.einsum('bhwc,bhwd->cd', xi[:, ky:ky + H, kx:kx + W], d) for kx in range(kf)]) for ky in range(kf)])
  return dw, d.sum(dim=(0, 1, 2))


def wgrad_ref_ups(x, du, kf):
  """The same for the stride-2 transposed conv that ran on x [B,Hs,Ws,Ci]: the autograd of deconv_ref with respect to its filter
  w [kf,kf,Co,Ci], returned in the KERNEL's layout [ky,kx,ci,co] of the equivalent plain conv (taps flipped, in / out swapped)."""
  Ci, Co = x.shape[3], du.shape[3]
  w = torch.zeros((kf, kf, Co, Ci), dtype=torch.float64, requires_grad=True)
  y = deconv_ref(x.double(), w, torch.zeros(Co, dtype=torch.float64), 2)
  (y * du.double()).sum().backward()
  return w.grad.flip(0, 1).permute(0, 1, 3, 2).contiguous(), du.double().sum(dim=(0, 1, 2))


# ---- the whole step: test_filter_sizes' sizes (stride-2 dcnn layers at 3, 5 and 1)
CTRL = [5, 3, 1, 3, 7, 3, 3, 3]
ATTN = [5, 3, 1, 3, 7, 3]
DCNN = [3, 5, 5, 7, 1, 3, 1]


def is_filter(k):
  tail = k.split('_')
  return 'w' in tail or (len(tail[-1]) == 3 and tail[-1][0] == 'w' and tail[-1][1] in 'xh')


def step_case(arch='cvppp', H=64, W=64, T=2, B=2, seed=3, wmul=0.6, **over):
  """test_train_gpu._case with the mixed filter sizes and train_any_filter.  25- and 49-tap filters raise the layer gains: a
  filter of size f is scaled by wmul * 3 / f (the 3x3 layers by wmul, as test_train_gpu does), which keeps every layer's gain
  (~ f * sigma) where the all-3x3 case has it.  The precondition — the oracle's own float32 run meets the bars against its
  float64 run on these inputs — is test_train_filter_sizes.py::test_step_inputs_are_well_conditioned."""
  filt = dict(ctrl_cnn_filter_size=CTRL)
  if arch != 'box':
    filt.update(attn_cnn_filter_size=ATTN, attn_dcnn_filter_size=DCNN)
  opt = ora.make_opt('cvppp' if arch == 'box' else arch, H, W, T, base_learn_rate=1e-3, learn_rate_decay=0.96,
                     steps_per_learn_rate_decay=5000, train_any_filter=True, **dict(filt, **over))
  P = ora.random_params(opt, seed, box_model=(arch == 'box'))
  rng = np.random.RandomState(seed + 100)
  sizes = {}
  for scope, key in (('ctrl_cnn', 'ctrl_cnn_filter_size'), ('attn_cnn', 'attn_cnn_filter_size'), ('attn_dcnn', 'attn_dcnn_filter_size')):
    sizes.update({'%s_w_%d' % (scope, i): f for i, f in enumerate(opt[key])})
  for k in P:
    if not is_filter(k):
      continue
    f = sizes.get(k, 3)
    if f == 3:
      P[k] = (P[k] * wmul).astype(np.float32)
    else:  # ora.random_params draws 3x3 filters: redraw at the configured size, with the 3x3 draw's spread times 3 / f
      P[k] = rng.normal(0.0, float(P[k].std()) * wmul * 3.0 / f, (f, f) + P[k].shape[2:]).astype(np.float32)
  rng = np.random.RandomState(seed + 1)
  x = rng.rand(B, H, W, 3).astype(np.float32)
  y_gt, s_gt = np.zeros((B, T, H, W), np.float32), np.zeros((B, T), np.float32)
  for b in range(B):
    y_gt[b, 0, H // 10:H // 2 - 2, W // 8:W // 2 + 2] = 1
    y_gt[b, 1, H // 2 + 4:H - 10, W // 2 - 2 + 2 * b:W - 4] = 1  # a different area: no tie in the greedy match
    s_gt[b, :2] = 1
  return opt, P, x, y_gt, s_gt


def oracle_grads(opt, P, x, y_gt, s_gt, noise=None):
  """Loss pieces, the gradient of every parameter and the batch statistics from ra_oracle_torch at its current precision
  (ort.deconv_same must already be deconv_ref).  noise: box_model's canvas-noise draws (then the box model's graph)."""
  keys = [k for k in P if not (k.endswith('_ema_mean') or k.endswith('_ema_var'))]
  stats = {}
  if noise is not None:
    head, Pt = ort.box_forward_loss(opt, P, x, y_gt, s_gt, noise, requires_grad=keys)
  else:
    fwd, Pt = ort.forward(opt, P, x, requires_grad=keys, phase_train=True, bn_stats=stats)
    head = ort.loss_head(opt, fwd, y_gt, s_gt)
  total = head['loss'] + ort.weight_decay_term(opt, {k: Pt[k] for k in keys})
  total.backward()
  grads = {k: Pt[k].grad.double().numpy() if Pt[k].grad is not None else np.zeros(P[k].shape) for k in keys}
  return head, grads, stats
