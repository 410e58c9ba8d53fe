"""Case tables of tests/test_attn_geometry.py (CPU) and tests/test_attn_geometry_gpu.py: the Gaussian-attention kernels over the
window geometries the controller can emit, and over the launch forms of the paste.

A 9-number attention record (ctr_y, ctr_x, size_y, size_x, lg_var_y, lg_var_x, attn gamma, box gamma, y lg gamma) fixes the two
filter banks of modellib.get_gaussian_filter: F taps at mu_j = ctr + (size + 1) / F * (j - (F - 1) / 2), each a Gaussian of
variance exp(lg_var) over the L pixels of its axis.  The kernels drop every weight below e^-30 of its tap's peak, i.e. keep tap
j on the pixels |l - mu_j| <= R = sqrt(60 exp(lg_var)).  Without squash_ctrl_params the centre and size are unbounded, fixed_var
sets lg_var = 0 whatever the size, dynamic_var makes it a raw network output: CLASSES names the resulting geometries of one
axis, RECORDS pairs them, SHAPES / FORM_ROWS say where they run and PASTE_CASES which paste kernel each GPU case is written for.

Everything here is NumPy on the host: the float64 references the GPU tests compare against, the float32 run of the same
dense operators (how well the reference is conditioned), the banded restatement of the kernels' rule and its three mutants.
"""
import functools

import numpy as np

import ra_oracle as ora

BETA = -5.0
B_LAUNCH = 6  # records per launch: one launch mixes classes

# ---- tolerances: the project's own (test_direct_extract_paste_box, test_banded_resample_adjoints_vs_dense_autograd)
TOL_EXTRACT = 3e-5  # x max(1, |ref|max)
TOL_PASTE = 2e-5    # y_out and canvas, absolute
TOL_BOX = 3e-5
TOL_ADJOINT = 1e-4  # x max(1, |g_ref|max), per parameter
CONDITIONING = 8.0  # the float32 reference, and the banding, sit at least this factor inside each tolerance


def _nat(s, F):
  return np.log(s / F)  # the model's own variance (get_normalized_var)


def _radius(lg_var):
  return np.sqrt(60.0 * np.exp(lg_var))


def _tail_only_lo(L, F):
  s = 0.3 * L
  return -(s / 2 + _radius(_nat(s, F)) / 2), s, _nat(s, F)


def _outside_lo(L, F):
  s = 0.3 * L
  return -(s / 2 + _radius(_nat(s, F)) + 3), s, _nat(s, F)


def _outside_hi(L, F):
  s = 0.3 * L
  return L + s / 2 + _radius(_nat(s, F)) + 3, s, _nat(s, F)


def _snapped(f):
  """The class f with its taps on float32-exact positions: ctr a multiple of 1/16 and (size + 1) / F a multiple of 1/64, so that
  every mu_j and every l - mu_j is exact in float32 as in float64.  A band of variance v turns an error e of mu into a relative
  error |l - mu| e / v of the weight: at lg_var = -6 one float32 rounding of a centre near 500 (3e-5) would be 0.4 % of a
  weight, far above any tolerance here, in the float32 reference as in the kernels.  That sensitivity belongs to the record, not
  to the code, so the narrow classes are placed where it does not enter."""
  def g(L, F):
    ctr, size, lg_var = f(L, F)
    return np.round(ctr * 16) / 16, F * max(np.round((size + 1) / F * 64), 1) / 64 - 1, lg_var
  return g


# id -> (L, F) -> (ctr, size, lg_var)
CLASSES = (
    ('inside', lambda L, F: (0.5 * L + 0.3, 0.4 * L, _nat(0.4 * L, F))),
    ('edge_lo', lambda L, F: (0.02 * L, 0.4 * L, _nat(0.4 * L, F))),
    ('edge_hi', lambda L, F: (0.97 * L, 0.4 * L, _nat(0.4 * L, F))),
    ('on_pixel0', lambda L, F: (0.0, 0.3 * L, _nat(0.3 * L, F))),
    ('on_last', lambda L, F: (L - 1.0, 0.3 * L, _nat(0.3 * L, F))),
    ('tail_only_lo', _tail_only_lo),   # only the tails of the taps nearest the image reach it
    ('outside_lo', _outside_lo),       # no band reaches the image
    ('outside_hi', _outside_hi),
    ('huge', lambda L, F: (0.45 * L, 3.0 * L, _nat(3.0 * L, F))),
    ('huge_var1', _snapped(lambda L, F: (0.45 * L, 3.0 * L, 0.0))),   # fixed_var: gaps between the bands
    ('subpixel', _snapped(lambda L, F: (0.5 * L + 0.3, 0.5, _nat(0.5, F)))),
    ('subpixel_var1', lambda L, F: (0.5 * L + 0.3, 0.5, 0.0)),
    ('wide', lambda L, F: (0.5 * L, 0.4 * L, _nat(0.4 * L, F) + 4.0)),
    ('wider_than_image', lambda L, F: (0.5 * L, 0.4 * L, 8.0)),
    ('narrow', _snapped(lambda L, F: (0.5 * L + 0.3, 0.4 * L, -3.0))),
    ('needle', _snapped(lambda L, F: (0.5 * L + 0.3, 0.4 * L, -6.0))),    # R < 0.5: most bands are empty
)
CLASS_IDS = tuple(c for c, _ in CLASSES)
_CLASS_FN = dict(CLASSES)
OUTSIDE = ('outside_lo', 'outside_hi')
PAIR_SHIFTS = (0, 5, 11)  # x class = y class shifted cyclically: every class on each axis three times, 48 records
MIN_SIZE = 0.25           # below, the float32 reference itself loses the tolerance (0.02 pixel: 1.6e-5 relative)

# ---- shapes: id -> (H, W, Fh, Fw).  Small on purpose; what each is for is in its comment
SHAPES = {
    's40x72': (40, 72, 16, 16),       # multiples of 4: the window paste kernel, all rows present
    's37x50': (37, 50, 16, 12),       # neither a multiple of 4, Fh != Fw: scalar stores, a short last block of the general kernel
    's64x64': (64, 64, 48, 48),       # the product's tap count
    's8x320': (8, 320, 4, 16),        # extract only: the huge x classes span more than 256 columns (two column pages)
    's6x1028': (6, 1028, 4, 16),      # W > 1024: the general paste kernel on float4 stores; five column pages of the extract
    's22x40': (22, 40, 8, 12),        # H % 4 = 2, W % 4 = 0: the window paste kernel with a short last block (nrow < RB)
}
EXTRACT_ONLY = ('s8x320',)
ADJOINT_SHAPES = {'a40x72': (40, 72, 16, 12), 'a37x50': (37, 50, 16, 12)}
# form-only rows: id -> (H, W, Fh, Fw), on the inside / edge_lo classes only
FORM_ROWS = {
    'f_fw80': (40, 72, 4, 80),        # extract parts = 2; paste general (Fw > 64)
    'f_fw130': (40, 72, 4, 130),      # extract parts = 1
    'f_64x64': (40, 72, 64, 64),      # Fh Fw > 3072: the patch plane does not fit the window kernel's staging
    'f_3x3': (40, 72, 3, 3),          # Fh Fw % 4 != 0
}
FORM_CLASSES = (('inside', 'inside'), ('inside', 'edge_lo'), ('edge_lo', 'inside'), ('edge_lo', 'edge_lo'), ('inside', 'edge_lo'),
                ('edge_lo', 'inside'))


def all_shapes():
  out = dict(SHAPES)
  out.update(FORM_ROWS)
  return out


def class_pairs(shape_id):
  """The (y class, x class) of every record of a shape, in launch order."""
  if shape_id in FORM_ROWS:
    return list(FORM_CLASSES)
  n = len(CLASS_IDS)
  return [(CLASS_IDS[i], CLASS_IDS[(i + s) % n]) for s in PAIR_SHIFTS for i in range(n)]


def _seed(shape_id):
  return sum(ord(c) * (i + 1) for i, c in enumerate(shape_id))


def records(shape_id, dims=None, skip=()):
  """(rec [N,16] float32, pairs): the records of a shape; gammas drawn as test_kernels_gpu._attn_rec draws them.
  skip: classes whose records are left out (N stays a multiple of B_LAUNCH by cycling the kept ones)."""
  H, W, Fh, Fw = dims or all_shapes()[shape_id]
  pairs = [p for p in class_pairs(shape_id) if p[0] not in skip and p[1] not in skip]
  k = 0
  while len(pairs) % B_LAUNCH:
    pairs.append(pairs[k])
    k += 1
  rng = np.random.RandomState(_seed(shape_id))
  rec = np.zeros((len(pairs), 16), np.float32)
  for k, (cy, cx) in enumerate(pairs):
    rec[k, 0], rec[k, 2], rec[k, 4] = _CLASS_FN[cy](float(H), float(Fh))
    rec[k, 1], rec[k, 3], rec[k, 5] = _CLASS_FN[cx](float(W), float(Fw))
  rec[:, 6] = rng.uniform(0.5, 2.0, len(pairs))
  rec[:, 7] = rng.uniform(0.5, 2.0, len(pairs))
  rec[:, 8] = rng.uniform(0.5, 2.5, len(pairs))
  assert (rec[:, 2:4] >= MIN_SIZE).all()
  return rec, pairs


# The patch that is pasted.  The paste's argument is z = e^g sum_ji fy(l,j) P[j,i] fx(w,i) + beta.  Its float32 rounding error, in
# the reference as in a kernel, is about 1e-7 x A |P| with A = e^g max_l sum_j fy max_w sum_i fx, and A runs from 0.1 (three taps on
# 40 pixels) to 700 (a needle's taps weigh 8 each) over the classes.  So the patch of record k is a normal draw scaled to
# PATCH_AMPL / A_k (at most PATCH_MAX): |z - beta| <~ PATCH_AMPL keeps the window in the sigmoid's live range for every class,
# where an error of the resample shows, and the rounding error the same small part of the tolerance.
PATCH_AMPL, PATCH_MAX = 4.0, 1.0


def is_outside(pair):
  return pair[0] in OUTSIDE or pair[1] in OUTSIDE


def inputs(shape_id, rec, dims=None, C=8):
  """The float32 operands every test of a shape shares: image [n,H,W,C] in [0,1), canvas [n,H,W] in [0,0.6), patch [n,Fh,Fw]
  (see PATCH_AMPL)."""
  H, W, Fh, Fw = dims or all_shapes()[shape_id]
  n = rec.shape[0]
  rng = np.random.RandomState(_seed(shape_id) + 1)
  img = rng.rand(n, H, W, C).astype(np.float32)
  canvas = rng.uniform(0, 0.6, (n, H, W)).astype(np.float32)
  r64 = rec.astype(np.float64)
  fy, fx = dense_banks(r64, H, W, Fh, Fw)
  ampl = np.exp(r64[:, 8]) * fy.sum(axis=2).max(axis=1) * fx.sum(axis=2).max(axis=1)
  scale = np.minimum(PATCH_AMPL / np.maximum(ampl, 1e-30), PATCH_MAX)
  P = (scale.reshape(-1, 1, 1) * rng.randn(n, Fh, Fw)).astype(np.float32)
  return img, canvas, P


# ---- the dense operators (the reference's formulation), in the dtype of their arguments
def dense_banks(rec, H, W, Fh, Fw):
  fy = ora.get_gaussian_filter(rec[:, 0], rec[:, 2], rec[:, 4], H, Fh)
  fx = ora.get_gaussian_filter(rec[:, 1], rec[:, 3], rec[:, 5], W, Fw)
  return fy, fx


def extract_op(img, fy, fx):
  """F_y^T X F_x per channel, [n,Fh,Fw,C] (no gamma)."""
  return ora.extract_patch(img, fy, fx, img.shape[3])


def resample_op(P, fy, fx):
  """F_y P F_x^T, [n,H,W]."""
  return np.matmul(np.matmul(fy, P), np.transpose(fx, (0, 2, 1)))


def _sigmoid(z):
  one = z.dtype.type(1)
  with np.errstate(over='ignore'):  # exp(-z) = inf gives the 0 it should
    return one / (one + np.exp(-z))


def paste_op(P, fy, fx, rec, beta=BETA):
  z = np.exp(rec[:, 8]).reshape(-1, 1, 1) * resample_op(P, fy, fx) + rec.dtype.type(beta)
  return _sigmoid(z)


def box_op(fy, fx, rec, beta=BETA):
  z = rec[:, 7].reshape(-1, 1, 1) * resample_op(np.ones((rec.shape[0], fy.shape[2], fx.shape[2]), rec.dtype), fy, fx) + rec.dtype.type(beta)
  return _sigmoid(z)


@functools.lru_cache(maxsize=None)
def reference(shape_id):
  """Everything the tests of one shape share, computed once and read-only: rec, pairs, the operands, the float64 banks and
  the float64 results of the three operators: extract [n,Fh,Fw,9] without gamma of the image's 8 channels and, as channel 8, of
  the canvas (the operator is linear: a canvas standing in for channel c is channel 8 in place of c); paste y before any
  canvas; box."""
  H, W, Fh, Fw = all_shapes()[shape_id]
  rec, pairs = records(shape_id)
  img, canvas, P = inputs(shape_id, rec)
  img_cv = np.concatenate([img, canvas[..., None]], axis=3)
  r64 = rec.astype(np.float64)
  fy, fx = dense_banks(r64, H, W, Fh, Fw)
  out = dict(rec=rec, pairs=tuple(pairs), img=img, canvas=canvas, P=P, img_cv=img_cv, fy=fy, fx=fx,
             extract=extract_op(img_cv.astype(np.float64), fy, fx), paste=paste_op(P.astype(np.float64), fy, fx, r64),
             box=box_op(fy, fx, r64), outside=np.array([is_outside(p) for p in pairs]))
  for v in out.values():
    if isinstance(v, np.ndarray):
      v.setflags(write=False)
  return out


# ---- the adjoints: the dense formulation under torch autograd (the construction of test_banded_resample_adjoints_vs_dense_autograd)
ADJOINT_PARAMS = ('ctr', 'size', 'lg_var', 'attn_gamma', 'box_gamma', 'y_lg_gamma', 'patch')


@functools.lru_cache(maxsize=None)
def adjoint_case(shape_id, with_needle=True):
  """rec, pairs and the float32 operands of an adjoint shape: image x [n,H,W,4], patch P, and the upstream gradients wE, wB, wY
  of the extract, the box and the paste."""
  dims = ADJOINT_SHAPES[shape_id]
  H, W, Fh, Fw = dims
  rec, pairs = records(shape_id, dims, skip=() if with_needle else ('needle',))
  img, _, P = inputs(shape_id, rec, dims, C=4)
  rng = np.random.RandomState(_seed(shape_id) + 2)
  n = rec.shape[0]
  out = dict(rec=rec, pairs=tuple(pairs), x=img, P=P, wE=rng.randn(n, Fh, Fw, 4).astype(np.float32),
             wB=rng.randn(n, H, W).astype(np.float32), wY=rng.randn(n, H, W).astype(np.float32), dims=dims)
  for v in out.values():
    if isinstance(v, np.ndarray):
      v.setflags(write=False)
  return out


def adjoint_reference(case, lo, hi, dtype):
  """Forward values and gradients of records lo:hi by torch autograd on the dense banks, in torch dtype `dtype`, on the host.
  Returns (fwd, grads): fwd = (e, box, y) arrays, grads = {parameter: [hi - lo, ...] array} of
  sum(e wE) + sum(box wB) + sum(y wY)."""
  import math
  import torch
  H, W, Fh, Fw = case['dims']
  t = lambda a: torch.tensor(np.array(a[lo:hi]), dtype=dtype)
  rec = t(case['rec'])
  leaves = [rec[:, 0:2], rec[:, 2:4], rec[:, 4:6], rec[:, 6], rec[:, 7], rec[:, 8], t(case['P'])]
  leaves = [a.clone().requires_grad_(True) for a in leaves]
  ctr, size, lgv, g_e, g_b, g_y, P = leaves
  banks = []
  for ax, (L, F) in enumerate(((H, Fh), (W, Fw))):
    j = torch.arange(F, dtype=dtype)
    mu = ctr[:, ax, None] + ((size[:, ax, None] + 1.0) / F) * (j[None, :] - (F - 1) / 2.0)
    dd = torch.arange(L, dtype=dtype)[None, :, None] - mu[:, None, :]
    var = torch.exp(lgv[:, ax])[:, None, None]
    banks.append(torch.exp(-0.5 * dd * dd / var) / (torch.sqrt(var) * math.sqrt(2 * math.pi)))
  fy, fx = banks
  e = g_e[:, None, None, None] * torch.einsum('blj,blwc,bwi->bjic', fy, t(case['x']), fx)
  bx = torch.sigmoid(g_b[:, None, None] * torch.einsum('blj,bwi->blw', fy, fx) + BETA)
  y = torch.sigmoid(torch.exp(g_y)[:, None, None] * torch.einsum('blj,bji,bwi->blw', fy, P, fx) + BETA)
  ((e * t(case['wE'])).sum() + (bx * t(case['wB'])).sum() + (y * t(case['wY'])).sum()).backward()
  return ([a.detach().numpy() for a in (e, bx, y)], {k: a.grad.numpy() for k, a in zip(ADJOINT_PARAMS, leaves)})


def adjoint_excess(got, ref):
  """Per record, the worst |got - ref| / (TOL_ADJOINT max(1, |ref|max)) over the parameters (each record and parameter on its
  own scale), and the parameter it is at."""
  n = ref['ctr'].shape[0]
  worst, at = np.zeros(n), [''] * n
  for k in ADJOINT_PARAMS:
    a, b = np.asarray(got[k], np.float64).reshape(n, -1), np.asarray(ref[k], np.float64).reshape(n, -1)
    r = np.abs(a - b).max(axis=1) / (TOL_ADJOINT * np.maximum(1.0, np.abs(b).max(axis=1)))
    r = np.where(np.isfinite(a).all(axis=1), r, np.inf)
    for i in np.flatnonzero(r > worst):
      worst[i], at[i] = r[i], k
  return worst, at


# ---- the kernels' banding rule restated in float64, and three wrong versions of it
MUTANTS = ('half_radius', 'half_is_F_over_2', 'step_without_plus_one')


def banded_bank(ctr, size, lg_var, L, F, mutant=None):
  """get_gaussian_filter in float64 with every weight below e^-30 of its tap's peak dropped (csrc/ra_attn_axis.h: the band of
  tap j is |l - mu_j| <= sqrt(60 var)).  mutant: one of MUTANTS."""
  assert mutant is None or mutant in MUTANTS
  ctr, size, lg_var = [np.asarray(a, np.float64).reshape(-1, 1, 1) for a in (ctr, size, lg_var)]
  j = np.arange(F, dtype=np.float64).reshape(1, 1, -1)
  half = F / 2.0 if mutant == 'half_is_F_over_2' else (F - 1) / 2.0
  step = size / F if mutant == 'step_without_plus_one' else (size + 1.0) / F
  mu = ctr + step * (j - half)
  var = np.exp(lg_var)
  R = np.sqrt(60.0 * var) * (0.5 if mutant == 'half_radius' else 1.0)
  d = np.arange(L, dtype=np.float64).reshape(1, L, 1) - mu
  w = np.exp(-0.5 * d * d / var) / np.sqrt(var) / np.sqrt(2 * np.pi)
  return np.where(np.abs(d) <= R, w, 0.0)


def banded_banks(rec, H, W, Fh, Fw, mutant=None):
  r = rec.astype(np.float64)
  return banded_bank(r[:, 0], r[:, 2], r[:, 4], H, Fh, mutant), banded_bank(r[:, 1], r[:, 3], r[:, 5], W, Fw, mutant)


# ---- which paste kernel each GPU case is written for.  A plan is named 'kernel rows last': last = 'full' when every workgroup
# holds `rows` image rows, 'short' when the last one holds fewer.  Variants of the launch's arguments:
#   plane     canvas in its own [B,H,W] plane, one-channel patch (the decode loop's launch)
#   chan      canvas as a channel of the packed image
#   packed    canvas plane, patch channel 2 of 4
#   nocanvas  no canvas at all (the training forward)
#   stride    plane, with y_out a view whose batch stride is not a multiple of 4
#   unaligned plane, with y_out 4 bytes off a 16-byte boundary
#   box       the attention box;  box_stride  the box into a view whose batch stride is not a multiple of 4
PASTE_VARIANTS = {
    'plane': dict(mode='paste', Cp=1, pc=0, has_canvas=True, has_img=False),
    'chan': dict(mode='paste', Cp=1, pc=0, has_canvas=False, has_img=True),
    'packed': dict(mode='paste', Cp=4, pc=2, has_canvas=True, has_img=False),
    'nocanvas': dict(mode='paste', Cp=1, pc=0, has_canvas=False, has_img=False),
    'stride': dict(mode='paste', Cp=1, pc=0, has_canvas=True, has_img=False, odd_stride=True),
    'unaligned': dict(mode='paste', Cp=1, pc=0, has_canvas=True, has_img=False, aligned16=False),
    'box': dict(mode='box'),
    'box_stride': dict(mode='box', odd_stride=True),
}
_GEN_FULL, _GEN_SHORT, _WIN_FULL, _WIN_SHORT = 'general r4 full', 'general r4 short', 'window r4 full', 'window r4 short'


def _row(shape_id, win):
  gen = _GEN_SHORT if all_shapes()[shape_id][0] % 4 else _GEN_FULL
  w = win or gen
  return {'plane': w, 'chan': gen, 'packed': gen, 'nocanvas': gen, 'stride': gen, 'unaligned': gen, 'box': w, 'box_stride': gen}


# shape id -> variant -> the plan the GPU case asserts before it launches
PASTE_CASES = {
    's40x72': _row('s40x72', _WIN_FULL),
    's37x50': _row('s37x50', None),       # W % 4 != 0
    's64x64': _row('s64x64', _WIN_FULL),
    's6x1028': _row('s6x1028', None),     # 4 rows x 1028 columns > 4096 floats
    's22x40': _row('s22x40', _WIN_SHORT),
    'f_fw80': _row('f_fw80', None),
    'f_fw130': _row('f_fw130', None),
    'f_64x64': _row('f_64x64', None),
    'f_3x3': _row('f_3x3', None),
}
# the form-only rows run the decode loop's two launches only
FORM_ROW_VARIANTS = ('plane', 'box')


def paste_variants(shape_id):
  return FORM_ROW_VARIANTS if shape_id in FORM_ROWS else tuple(PASTE_VARIANTS)


def odd_stride(H, W):
  """A batch stride (floats) of a [B, 2, H, W]-like view that is not a multiple of 4."""
  s = 2 * H * W + 1
  return s if s % 4 else s + 1


def paste_plan_str(shape_id, variant, aligned16=None):
  """'kernel rows last' of the plan ra_paste_plan returns for a variant of a shape (host only)."""
  import ra_ops as ops
  H, W, Fh, Fw = all_shapes()[shape_id]
  v = dict(PASTE_VARIANTS[variant])
  stride = odd_stride(H, W) if v.pop('odd_stride', False) else 2 * H * W
  if aligned16 is None:
    aligned16 = v.pop('aligned16', True) and (H * W) % 4 == 0   # the tests write plane 1 of a [B,2,H,W] buffer
  else:
    v.pop('aligned16', None)
  p = ops.paste_plan(v.pop('mode'), B_LAUNCH, H, W, Fh, Fw, y_stride_b=stride, aligned16=aligned16, **v)
  assert p['threads'] == 256 and p['grid_x'] == -(-H // p['rows'])
  return '%s r%d %s' % (p['kernel'], p['rows'], 'short' if H % p['rows'] else 'full')
