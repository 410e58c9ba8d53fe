"""The decode-loop engine: the T-step recurrent-attention forward of full_model / box_model
driven through the C ABI, with every buffer pre-allocated and the whole launch sequence
replayable as one HIP graph.

Per output timestep tt (full_model.py:638-848), all on one stream:
   K1 x L   ctrl CNN   conv3x3+bias+BN(tt)+ReLU+pool  (f32 MFMA)      img -> feat [B,G,Cf]
   K2       controller glimpse/LSTM/gMLP x iters, cMLP, attn decode  feat -> attn record
   K3       extract    gamma * fy^T X fx                             img -> x_patch
   K4 x ..  attn CNN / DCNN (same MFMA conv kernel; transposed packing + zero-stuffing + skip)
   K6       score      sigmoid([h, h_core] w + b)                    -> s_out[:, tt]
   K5       paste      sigmoid(e^g fy P fx^T - 5)(1-canvas), canvas = max -> y_out[:, tt], img
`img` is the packed NHWC image [x | canvas slot | d_in | y_in | 0-pad]; the canvas itself lives in its own
[B,H,W] plane that the first controller-CNN layer and the extract kernel substitute for the slot.
"""
import numpy as np
import math
import os

import torch

import operator

import ra_native as rn
import ra_ops as ops


def _dev(a, device):
  return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _r4(n):
  return -(-n // 4) * 4


_TENSOR_VERSION = operator.attrgetter('_version')


class DecodeEngine(object):
  """dims: the derived shape/flag dict (full_model.derive_dims); model: name -> tensor."""

  def __init__(self, dims, model, box_model=False):
    self.d = dims
    self.model = model
    self.box = box_model
    self._stamp = None
    self._B = None
    self._graphs = {}
    self.fuse_pairs = True  # fused two-layer conv launches in the controller CNN where it pays
    self.fuse_patch_pairs = False  # ... and in the patch-sized attention CNN / DCNN (it does not)
    self.ctrl_split = True  # 16-workgroup LDS-stationary controller where supported
    self.fuse_score = True  # score MLP as an extra workgroup of the paste launch
    # ... also where that splits a fused pair (the 16 -> 16 layer of L2+L3)?  Measured at cfg2: L2 direct 20.6 +
    # L3 Winograd 22.2 us against 41.8 us fused: no gain, one more launch -> off
    self.wino_unfuse = False
    self.pair_wino = True  # the fused L2+L3 pair with its second layer as Winograd (K1pw)
    # ... or, first, with both layers direct on the bf16 matrix pipe (K1p16); RA_PAIR16=0: K1pw.  pair_wino = False switches both off
    self.pair_direct16 = os.environ.get('RA_PAIR16', '1') != '0'
    self.use_wino = True  # controller-CNN layers with Cin 16 | 32, Cout % 32 == 0 as Winograd F(2x2,3x3) (K1w)
    self.cache_first = True  # image part of the first controller-CNN layer cached once per forward
    self.fill_cache_inline = True  # ... by the first timestep's own launch (else: a separate kernel)
    self.co_resident = 1  # engines decoding concurrently on this GPU (set by full_model.DecodePipeline)
    # drawn tiles in the controller CNN's persistent launches (ra_tile_tickets_bind): for a GPU this process does NOT own.  With
    # another stream's controllers as company the launch group slows x1.12-1.21 instead of x1.37 (tools/contention_probe.py);
    # inside our own decode pipeline it measured neutral (63.7k vs 64.0k: profiles/r05_tile_tickets.txt), hence off by default.
    self.tile_tickets = os.environ.get('RA_ENGINE_TICKETS', '0') != '0'
    self.nsub = 0  # sub-batches decoded on parallel streams; 0 = one (see _launch_all)
    self.use_graph = True
    self.prefill_ride = True  # the once-per-forward y_out prefill rides on the first controller-CNN launch
    self.use_split = os.environ.get('RA_USE_SPLIT', '1') != '0'  # K1s: the mid-resolution controller-CNN layers as direct convs on the bf16 matrix pipe at float32 accuracy
    # round 6: K1s also as the FIRST controller-CNN layer where no image-part cache applies (the KITTI / Cityscapes architectures:
    # 13 / 21 channels packed to 16 / 24, the canvas as a plane — ra_conv_split_plane_f32) ...
    self.split_first = os.environ.get('RA_SPLIT_FIRST', '1') != '0'
    self.ctrl_batch_xcd = os.environ.get('RA_CTRL_BATCH_XCD', '1') != '0'  # K2b's groups each on an XCD of their own, exchanging through its L2
    self.xcd_slot, self.xcd_slots = 0, 1  # this engine's place among the launches that can run at the same time (set by DecodePipeline; 0 slots: unknown company -> agent scope)
    self.box_iou_rects = os.environ.get('RA_BOX_IOU_RECTS', '1') != '0'  # box_model: IoU of the step's box against the GT boxes from their corners
    # ... and in the attention CNN on the 48 x 48 patch (single-source layers with 16 / 24 / 32 / 64 input channels; ragged 24- and
    # 12-pixel maps).  'auto': where a layer has >= RA_SPLIT_PATCH_MIN_MF MFLOP per launch (the KITTI-sized nets: 16 images x 5-40
    # MFLOP), not the CVPPP net's sub-MFLOP layers, which are launch-latency-bound and lose to K1s's filter copy
    self.split_patch = os.environ.get('RA_SPLIT_PATCH', 'auto')
    # extract + attention-CNN layer 0 as one launch (ra_extract_conv0_f32, round 5): built, parity-tested and MEASURED SLOWER than
    # the two launches it replaces (11.8 vs 7.1 + 3.5 us at cfg2, profiles/r05_attn_fusion_probe.txt) — off; RA_FUSE_EXTRACT_CONV0=1 runs it
    self.fuse_extract_conv0 = os.environ.get('RA_FUSE_EXTRACT_CONV0', '0') == '1'
    self.timing = None  # set to a list to collect (stage, start_event, end_event)

  # ------------------------------------------------------------------ weights
  def _weights_stamp(self):
    """Changes whenever a weight does.  full_model.Model counts the mutations of the dict itself (`_mut`: an entry replaced,
    added, removed); in-place edits show in the tensors' version counters, whose sum only grows — one C-level pass over a
    cached list (~0.1 ms for cfg2's 1 400 tensors; the (key, pointer, version) tuple it replaces took 0.6 ms per forward, which
    made the HOST the bound of the four-slot pipeline).  A plain dict as the model keeps the full tuple."""
    m = self.model
    mut = getattr(m, '_mut', None)
    if mut is None:
      return tuple((k, v.data_ptr(), v._version) for k, v in sorted(m.items())
                   if isinstance(v, torch.Tensor) and '_' in k and not k.startswith('__'))
    if getattr(self, '_wlist_mut', None) != mut:
      self._wlist = [v for k, v in sorted(m.items()) if isinstance(v, torch.Tensor) and '_' in k and not k.startswith('__')]
      self._wlist_mut = mut
    return (mut, sum(map(_TENSOR_VERSION, self._wlist)))

  def _chan_map(self, flags):
    """packed channel -> index in the reference's concat order (full_model.py:640-661) or -1."""
    d = self.d
    groups = [(d['D'], True, flags[0]), (1, True, flags[1]), (8, d['add_d_out'], flags[2]),
              (d['nsc'], d['add_y_out'], flags[3])]
    cmap, idx = [], 0
    for n, present, used in groups:
      if not present:
        if used:
          raise rn.RecAttendError('input group used by the model but not fed')
        continue
      for _ in range(n):
        if used:
          cmap.append(idx)
          idx += 1
        else:
          cmap.append(-1)
    cmap += [-1] * (d['C0p'] - len(cmap))
    return cmap, idx

  def prepare(self, device):
    stamp = self._weights_stamp()
    if stamp == self._stamp:
      return
    d, M, T = self.d, self.model, self.d['T']
    bn = lambda scope, i, t: tuple(M['%s_%d_%d_%s' % (scope, i, t, n)]
                                   for n in ('beta', 'gamma', 'ema_mean', 'ema_var'))

    def fold_all(scope, i, cout):
      sc, sh = [], []
      for t in range(T):
        a, b = ops.fold_bn(M['%s_b_%d' % (scope, i)], cout, bn(scope, i, t) if d['use_bn'] else None)
        sc.append(a)
        sh.append(b)
      return _dev(np.stack(sc), device), _dev(np.stack(sh), device)

    W = {}
    # filter size per layer (nnlib.cnn / dcnn take one each): a layer of another size than 3 packs with its own and always runs
    # on ra_convkxk_f32 — none of the 3x3 forms (Winograd, K1s, fused pairs, the first layer's image cache, extract + conv0)
    ks = self.ksize = {'ccnn': list(d['ccnn_filters'])}
    if not self.box:
      ks['acnn'], ks['adcnn'] = list(d['acnn_filters']), list(d['adcnn_filters'])
    cmap_c, n_c = self._chan_map(d['ctrl_in'])
    assert n_c == d['ccnn_channels'][0]
    W['ccnn'], W['ccnn_wino'], W['ccnn_split'] = [], [], []
    hh, ww = d['H'], d['W']
    for i in range(d['ccnn_nlayers']):
      cin, cout = d['ccnn_channels'][i], d['ccnn_channels'][i + 1]
      k3 = ks['ccnn'][i] == 3
      if i == 0:
        wp = ops.pack_conv_weights(M['ctrl_cnn_w_0'], cin_kernel=d['C0p'], chan_map=cmap_c)
      else:
        wp = ops.pack_conv_weights(M['ctrl_cnn_w_%d' % i], cin_kernel=_r4(cin))
      sc, sh = fold_all('ctrl_cnn', i, cout)
      W['ccnn'].append((_dev(wp, device), sc, sh, cout, d['ccnn_pool'][i]))
      # mid-resolution layers also as Winograd F(2x2,3x3) filters (K1w: 2.25x fewer MFMAs), where the shape allows
      wino = i > 0 and k3 and self.use_wino and ops.conv_wino_supported(cin, cout, d['ccnn_pool'][i], hh, ww)
      W['ccnn_wino'].append(_dev(ops.pack_wino_weights(M['ctrl_cnn_w_%d' % i]), device) if wino else None)
      # ... and as the exact three-piece bf16 split of the filter, for the direct form on the bf16 matrix pipe (K1s, round 5)
      # Cin >= 32: always.  Cin = 16: where Winograd does not take the layer; and, round 6, where the layer has 16 output channels —
      # K1s then runs two workgroups per CU (Geo::OCC) with two windows in flight and beats K1w (KITTI's L1, 16 -> 16 pool 2:
      # 12.4 -> 10.1 us at cfg3, 8.1 -> 6.8 at cfg5); 16 -> 32 stays with K1w (cfg2's L4 12.3 vs 12.9 us, cfg5's L2 6.0 vs 7.1:
      # profiles/r06_k1s_sweep.txt)
      split = (i > 0 and k3 and self.use_split and (cin >= int(os.environ.get('RA_SPLIT_MIN_CIN', '32')) or not wino or cout == 16) and
               ops.conv_split_supported(_r4(cin), cout, d['ccnn_pool'][i], hh, ww))
      if (i == 0 and k3 and self.use_split and self.split_first and d['C0p'] != 4 and
          ops.conv_split_supported(d['C0p'], cout, d['ccnn_pool'][0], hh, ww)):
        W['ccnn_split'].append(torch.from_numpy(ops.pack_split_weights(M['ctrl_cnn_w_0'], cin_kernel=d['C0p'], chan_map=cmap_c)).to(device))
      else:
        W['ccnn_split'].append(torch.from_numpy(ops.pack_split_weights(M['ctrl_cnn_w_%d' % i])).to(device) if split else None)
      hh, ww = hh // d['ccnn_pool'][i], ww // d['ccnn_pool'][i]
    Cf = d['ccnn_channels'][-1]
    self.desc = ops.make_ctrl_desc(d['G'], Cf, d['hid'], d['iters'], d['n_gmlp'], d['n_cmlp'],
                                   d['mlp_dim'], d['H'], d['W'], d['Fh'], d['Fw'], d['squash'],
                                   d['fixed_var'], d['dynamic_var'],
                                   d.get('fixed_gamma', True))
    lstm = {k: M['ctrl_lstm_' + k] for k in ('w_xi', 'w_hi', 'b_i', 'w_xf', 'w_hf', 'b_f', 'w_xu',
                                             'w_hu', 'b_u', 'w_xo', 'w_ho', 'b_o')}
    gm = [(M['glimpse_mlp_w_%d' % i], M['glimpse_mlp_b_%d' % i]) for i in range(d['n_gmlp'])]
    cm = [(M['ctrl_mlp_w_%d' % i], M['ctrl_mlp_b_%d' % i]) for i in range(d['n_cmlp'])]
    W['ctrl'] = _dev(ops.pack_ctrl_weights(self.desc, lstm, gm, cm), device)
    self.split_ok = self.ctrl_split and ops.ctrl_split_supported(self.desc)
    if self.split_ok:
      W['ctrl_split'] = _dev(ops.pack_ctrl_split_weights(self.desc, lstm, gm, cm), device)
    W['smlp_w'] = M['score_mlp_w_0']
    W['smlp_b'] = M['score_mlp_b_0']
    if not self.box:
      cmap_a, n_a = self._chan_map(d['attn_in'])
      assert n_a == d['acnn_channels'][0]
      self.attn_sel = [c for c, m in enumerate(cmap_a) if m >= 0]
      W['acnn'], W['acnn_split'] = [], []
      ph, pw = d['Fh'], d['Fw']
      for i in range(d['acnn_nlayers']):
        cin, cout = d['acnn_channels'][i], d['acnn_channels'][i + 1]
        if i == 0:
          wp = ops.pack_conv_weights(M['attn_cnn_w_0'], cin_kernel=d['C0p'], chan_map=cmap_a)
        else:
          wp = ops.pack_conv_weights(M['attn_cnn_w_%d' % i], cin_kernel=_r4(cin))
        sc, sh = fold_all('attn_cnn', i, cout)
        W['acnn'].append((_dev(wp, device), sc, sh, cout, d['acnn_pool'][i]))
        ck = d['C0p'] if i == 0 else _r4(cin)
        k3 = ks['acnn'][i] == 3
        sp = None
        if k3 and self.use_split and self.split_patch != '0' and ops.conv_split_supported(ck, cout, d['acnn_pool'][i], ph, pw):
          mf = 2e-6 * 9 * cin * cout * ph * pw  # MFLOP per image
          if self.split_patch == '1' or mf >= float(os.environ.get('RA_SPLIT_PATCH_MIN_MF', '4')):
            sp = torch.from_numpy(ops.pack_split_weights(M['attn_cnn_w_%d' % i], cin_kernel=ck, chan_map=cmap_a if i == 0 else None)).to(device)
        W['acnn_split'].append(sp)
        ph, pw = ph // d['acnn_pool'][i], pw // d['acnn_pool'][i]
        if i == 0 and k3 and ops.extract_conv0_supported(d['C0p'], d['Fh'], d['Fw'], cout, d['acnn_pool'][0]):
          # the layer's filter in the PACKED input's channel order, for the launch that fuses it into the extract
          w0 = M['attn_cnn_w_0'].detach().cpu().numpy().astype(np.float32)
          plain = np.zeros((3, 3, d['C0p'], cout), np.float32)
          for c, m_ in enumerate(cmap_a):
            if m_ >= 0:
              plain[:, :, c, :] = w0[:, :, m_, :]
          W['acnn0_plain'] = _dev(plain, device)
      # DCNN: filter input channels = [prev | skip] (nnlib.py:365); skip sources are
      # [None, h_acnn[L-2], ..., h_acnn[0], x_patch] gated by the reversed skip flags
      # (full_model.py:494-499,798-803)
      W['adcnn'] = []
      L = d['acnn_nlayers']
      prev_c = d['adcnn_channels'][0]
      for i in range(d['adcnn_nlayers']):
        cout = d['adcnn_channels'][i + 1]
        n_skip = d['skip_ch'][i] if d['skip_ch'] is not None else 0
        src = None  # index into the skip source list
        if n_skip:
          src = i - 1  # 0 -> h_acnn[L-2], ..., L-1 -> x_patch
        c_prev = _r4(prev_c)
        cmap = [k if k < prev_c else -1 for k in range(c_prev)]
        c_skip = 0
        if src is not None:
          if src == L - 1:  # x_patch: packed channel order
            cmap += [prev_c + m if m >= 0 else -1 for m in cmap_a]
            c_skip = d['C0p']
          else:
            sc_real = d['acnn_channels'][L - 1 - src]
            c_skip = _r4(sc_real)
            cmap += [prev_c + k if k < sc_real else -1 for k in range(c_skip)]
        wp = ops.pack_conv_weights(M['attn_dcnn_w_%d' % i], cin_kernel=c_prev + c_skip,
                                   chan_map=cmap, transposed=True)
        sc, sh = fold_all('attn_dcnn', i, cout)
        W['adcnn'].append((_dev(wp, device), sc, sh, cout, d['adcnn_unpool'][i], src))
        prev_c = cout
    self.W = W
    self.plan = self._make_plan(W)
    self._stamp = stamp
    self._graphs = {}
    for k, (g_, s_, st_, _) in list(self.__dict__.get('_states', {}).items()):  # the parked sizes' graphs hold the old packs too
      self._states[k] = (g_, s_, st_, {})

  def _make_plan(self, W):
    """Greedy pairing of consecutive conv layers into fused launches (ra_conv_pair_f32): A must
    not pool (cnn) / B must not upsample (dcnn), single source, channel counts supported."""
    d = self.d
    plan = {}

    def pair_up(n, cin, cout, a_ok, b_ok, unfuse=lambda i: False, ks=None):
      steps, i = [], 0
      while i < n:
        # measured on MI355X: fusion pays while the intermediate has <= 16 channels (LDS tile
        # small enough for a 16x32 tile); wider pairs recompute too much halo.  3x3 layers only
        if (self.fuse_pairs and i + 1 < n and ks[i] == 3 and ks[i + 1] == 3 and a_ok(i) and b_ok(i + 1) and cout(i) <= 16 and
            ops.conv_pair_supported(cin(i), cout(i), cout(i + 1)) and not unfuse(i + 1)):
          steps.append(('pair', i, i + 1))
          i += 2
        else:
          steps.append(('single', i))
          i += 1
      return steps

    cc = d['ccnn_channels']
    # a layer that can run as Winograd (K1w) is worth more alone than as the second half of a fused pair
    wino_alone = lambda i: self.use_wino and self.wino_unfuse and W['ccnn_wino'][i] is not None
    plan['ccnn'] = pair_up(d['ccnn_nlayers'], lambda i: d['C0p'] if i == 0 else _r4(cc[i]),
                           lambda i: cc[i + 1], lambda i: d['ccnn_pool'][i] == 1, lambda i: True, wino_alone, ks=self.ksize['ccnn'])
    if not self.box:
      ac = d['acnn_channels']
      L = d['acnn_nlayers']
      # attn-CNN outputs that feed DCNN skip connections must be materialised (not fused away)
      skip_used = set(L - 2 - lay_[5] for lay_ in W['adcnn'] if lay_[5] is not None and lay_[5] < L - 1)
      fuse_patch = self.fuse_patch_pairs
      plan['acnn'] = pair_up(L, lambda i: d['C0p'] if i == 0 else _r4(ac[i]), lambda i: ac[i + 1],
                             lambda i: fuse_patch and d['acnn_pool'][i] == 1 and i not in skip_used,
                             lambda i: True, ks=self.ksize['acnn'])
      dc = d['adcnn_channels']
      lay = W['adcnn']
      plan['adcnn'] = pair_up(d['adcnn_nlayers'], lambda i: _r4(dc[i]), lambda i: dc[i + 1],
                              lambda i: fuse_patch and lay[i][5] is None,
                              lambda i: lay[i][5] is None and lay[i][4] == 1, ks=self.ksize['adcnn'])
    return plan

  # ------------------------------------------------------------------ buffers
  def alloc(self, B, device):
    """Buffers for a batch of B split into `nsub` independent sub-batches (each decoded on its
    own HIP stream: the latency-bound controller / patch kernels of one sub-batch overlap the
    other's conv launches).  Batch-leading tensors are shared and sliced; the rest is per
    sub-batch."""
    nsub = self.nsub if self.nsub else 1
    if B % nsub:
      nsub = 1
    if self._B == (B, nsub):
      return
    # a few batch sizes stay allocated (buffers AND captured graphs): a pipeline slot that decodes 2 x 8 images in the steady
    # state and lone batches of 8 at the end of a stream (DecodePipeline._ends_soon), or an evaluator's ragged last batch, must
    # not re-allocate and re-capture at every change of size
    states = self.__dict__.setdefault('_states', {})
    if self._B is not None:
      states[self._B] = (self.glob, self.subs, self.streams, self._graphs)
      while len(states) > 3:
        states.pop(next(iter(states)))
    hit = states.pop((B, nsub), None)
    if hit is not None:
      self.glob, self.subs, self.streams, self._graphs = hit
      self._B = (B, nsub)
      return
    d, T = self.d, self.d['T']
    f = lambda *s: torch.zeros(s, dtype=torch.float32, device=device)
    H, W, Fh, Fw = d['H'], d['W'], d['Fh'], d['Fw']
    g = {}
    g['x'] = f(B, H, W, d['D'])
    if d['add_d_out']:
      g['d_in'] = f(B, H, W, 8)
    if d['add_y_out']:
      g['y_in'] = f(B, H, W, d['nsc'])
    g['s_out'] = f(B, T) if (self.box is False or d['nsc'] == 1) else f(B, T, d['nsc'])
    g['attn_box'] = f(B, T, H, W)
    if self.box:
      g['y_gt'] = f(B, T, H, W)
      g['noise'] = f(T, B, H, W)
    else:
      g['y_out'] = f(B, T, H, W)
    Bs = B // nsub
    subs = []
    for k in range(nsub):
      b = {kk: v[k * Bs:(k + 1) * Bs] for kk, v in g.items() if kk != 'noise'}
      b['img'] = f(Bs, H, W, d['C0p'])
      b['canvas'] = f(Bs, H, W)
      hh, ww = H, W
      b['ccnn'] = []
      for i in range(d['ccnn_nlayers']):
        hh, ww = hh // d['ccnn_pool'][i], ww // d['ccnn_pool'][i]
        b['ccnn'].append(f(Bs, hh, ww, d['ccnn_channels'][i + 1]))
      b['tickets'] = ops.tickets_alloc(16 * T, device)  # <= 16 ticketed launch slices per timestep
      b['h_last'] = f(T, Bs, d['hid'])
      b['ctrl_out'] = f(T, Bs, 9)
      b['gmaps'] = f(T, Bs, d['iters'], d['G'])
      b['attn'] = f(T, Bs, rn.RA_ATTN_STRIDE)
      st0 = self.plan['ccnn'][0]
      if self.cache_first and st0[0] == 'pair' and d['C0p'] == 4 and self.ksize['ccnn'][:2] == [3, 3] and \
          ops.first_cache_supported(4, d['ccnn_channels'][1], d['ccnn_channels'][2], d['ccnn_pool'][1], H, W):
        b['l0cache'] = ops.first_cache_alloc(Bs, H, W, device)
      # `co_resident` = how many such launches may overlap (DecodePipeline: its depth)
      form = ops.ctrl_form(self.desc, Bs, self.co_resident) if self.split_ok else None
      if form == 'split':
        b['ctrl_ws'], b['ctrl_status'] = ops.ctrl_split_workspace(self.desc, Bs, device)
      elif form == 'batch':  # the group-shared form (K2b, 16 workgroups per group of images)
        b['ctrl_ws'], b['ctrl_status'] = ops.ctrl_batch_workspace(self.desc, Bs, device)
        b['ctrl_batch'] = True
        # round 6: K2b on the XCD-local exchange where every group of every launch that can run at the same time gets an XCD
        # of its own: `xcd_slot` of `xcd_slots` concurrent launches (DecodePipeline: stream k of its streams; a lone engine: 0 of 1)
        ng = -(-Bs // ops.ctrl_batch_group(self.desc, Bs))
        # ... and the teams in flight take at most half of the XCDs (RA_CTRL_BATCH_XCD_MAX_TEAMS, default 4).  Measured: cfg5's two
        # slots of two groups 42.5k -> 45.5k instance-timesteps/s (the tail as launched 284 -> 279 us and, more, 16 CUs of ONE XCD
        # per team instead of 4 on each of the eight); cfg2's four slots of two groups 68.0k -> 65.6k: with a team on every XCD the
        # controller CNN's XCD-contiguous tile walks each wait for a half-occupied XCD somewhere (profiles/r06_k1s_sweep.txt)
        if self.ctrl_batch_xcd and self.xcd_slots >= 1 and self.xcd_slots * ng <= int(os.environ.get('RA_CTRL_BATCH_XCD_MAX_TEAMS', '4')):
          b['ctrl_xcd_off'] = (self.xcd_slot % self.xcd_slots) * ng
      if self.box:
        b['noise'] = f(T, Bs, H, W)
        b['ysel'] = f(Bs, H, W)
        b['match'] = f(Bs, T)
        b['box1'] = f(Bs, 1, H, W)
      else:
        b['x_patch'] = f(T, Bs, Fh, Fw, d['C0p'])
        hh, ww = Fh, Fw
        b['acnn'] = []
        for i in range(d['acnn_nlayers']):
          hh, ww = hh // d['acnn_pool'][i], ww // d['acnn_pool'][i]
          b['acnn'].append(f(Bs, hh, ww, d['acnn_channels'][i + 1]))
        b['adcnn'] = []
        for i in range(d['adcnn_nlayers']):
          hh, ww = hh * d['adcnn_unpool'][i], ww * d['adcnn_unpool'][i]
          if i == d['adcnn_nlayers'] - 1:
            b['y_out_patch'] = f(T, Bs, hh, ww, d['adcnn_channels'][i + 1])
            b['adcnn'].append(None)
          else:
            b['adcnn'].append(f(Bs, hh, ww, d['adcnn_channels'][i + 1]))
      subs.append(b)
    self.glob = g
    self.subs = subs
    self.streams = [torch.cuda.Stream(device=device) for _ in range(nsub)] if nsub > 1 else []
    self._B = (B, nsub)
    self._graphs = {}

  def fetch(self, name):
    """A result buffer for the whole batch: shared tensors directly, per-sub-batch [T,Bs,...]
    buffers concatenated along their batch dimension."""
    if name in self.glob:
      return self.glob[name]
    parts = [sb[name] for sb in self.subs]
    if len(parts) == 1:
      return parts[0]
    dim = 0 if name in ('img', 'canvas') else 1
    return torch.cat(parts, dim=dim)

  def check_status(self, recover=True):
    """After the forward has finished: the 16-workgroup controller's status words.  Non-zero means a
    workgroup waited for a peer that never became resident (ra_ctrl_split.hip, kSpinLimit: something
    else held the CUs the residency rule counted on) and the outputs of that forward are garbage.
    recover: decode the same inputs again, synchronously, on the one-workgroup controller (no
    cross-workgroup waits at all) — this engine keeps that controller from then on — and warn; False:
    raise.  Returns True when a recovery ran."""
    bad = False
    for sb in self.subs:
      st = sb.get('ctrl_status')
      if st is not None and int(st.item()) != 0:
        st.zero_()
        bad = True
    if not bad:
      return False
    if not recover:
      raise rn.RecAttendError('controller_split: a workgroup timed out waiting for its peers (the launch was '
                              'not fully resident); decode with engine.ctrl_split = False')
    import warnings
    warnings.warn('controller_split: a workgroup timed out waiting for its peers (the launch was not fully resident: is '
                  'something else using this GPU?); the batch is decoded again on the one-workgroup controller, which this '
                  'engine keeps from now on')
    torch.cuda.synchronize()
    keep = {k: self.glob[k].clone() for k in ('x', 'd_in', 'y_in', 'y_gt', 'noise') if k in self.glob}
    want_box = getattr(self, '_last_want_box', False)
    self.ctrl_split = False
    self._stamp = None   # prepare() again: split_ok becomes False
    self._B = None       # alloc() again: no exchange workspace, so _launch_tail takes ra_controller_f32
    self._states = {}
    self._graphs = {}
    self.forward(keep['x'], d_in=keep.get('d_in'), y_in=keep.get('y_in'), y_gt=keep.get('y_gt'), noise=keep.get('noise'),
                 want_box=want_box)
    torch.cuda.synchronize()
    return True

  # ------------------------------------------------------------------ launch sequence
  def _mark(self, name):
    if self.timing is not None:
      ev = torch.cuda.Event(enable_timing=True)
      ev.record()  # on the current stream = the stream every kernel here is launched on
      self.timing.append((name, ev))

  def stage_times_ms(self):
    """After a forward with self.timing = [] and a synchronize: {stage: (total ms, launches)}
    from the HIP events recorded between stages."""
    out = {}
    for (_, e0), (name, e1) in zip(self.timing[:-1], self.timing[1:]):
      tot, n = out.get(name, (0.0, 0))
      out[name] = (tot + e0.elapsed_time(e1), n + 1)
    return out

  def _launch_all(self, want_box):
    """All sub-batches; with more than one, each on its own stream forked from / joined to the
    current stream (inside a graph capture this becomes parallel branches)."""
    if len(self.subs) == 1:
      self._launch_sub(self.subs[0], want_box)
      return
    main = torch.cuda.current_stream()
    for sb, st in zip(self.subs, self.streams):
      st.wait_stream(main)
      with torch.cuda.stream(st):
        self._launch_sub(sb, want_box)
    # (Measured, DESIGN.md §5: the branches run in lockstep, so two sub-batches are within 1 % of
    #  one; making their conv phases mutually exclusive — graph edges added after capture,
    #  per-timestep graphs chained by events, or linear graphs with device-side semaphores — was
    #  slower every time on ROCm 7.2, and a branched graph costs the host ~2 ms per replay against
    #  0.15 ms for the linear one.  Hence nsub defaults to 1.)
    for st in self.streams:
      main.wait_stream(st)

  def _launch_sub(self, b, want_box):
    self._launch_pack(b)
    # the controller CNN's persistent launches draw their tiles (ra_tile_tickets_bind): another slot's controller or patch
    # convs on the same GPU then cost them their share of the chip, not a second round (tools/contention_probe.py)
    bound = self.tile_tickets and 'tickets' in b and ops.tickets_bind(b['tickets'])
    try:
      for tt in range(self.d['T']):
        self._launch_tail(b, tt, want_box, self._launch_encoder(b, tt))
    finally:
      if bound:
        ops.tickets_unbind()

  def _launch_encoder(self, b, tt):
    fill = b['y_out'] if (tt == 0 and b.pop('_fill_rider', False)) else None
    return self._run_cnn(self.plan['ccnn'], self.W['ccnn'], b['img'], b['ccnn'], tt, 'ctrl_cnn',
                         plane=b['canvas'], cache=b.get('l0cache'), fill=fill)

  def _prefill_rides(self, b):
    """The y_out prefill can travel on the first timestep's cache-filling pair launch."""
    st0 = self.plan['ccnn'][0]
    return (self.prefill_ride and 'l0cache' in b and self.fill_cache_inline and st0[0] == 'pair' and
            ops.fill_rider_ok(b['y_out']))

  def _launch_pack(self, b):
    if self._prepacked:  # fg_model's head wrote b['img'] (forward(prepacked=True)); the canvas starts at zero in every forward
      b['canvas'].zero_()
    else:
      ops.pack_input(b['x'], b.get('d_in'), b.get('y_in'), self.d['C0p'], b['img'],
                     canvas_plane=b['canvas'])  # canvas = 0 (full_model.py:239) in the same pass
    if not self.box and not self.d['disable_overwrite']:
      # every pixel outside an attention window is sigmoid(0 - 5) (full_model.py:813-818): fill
      # once per forward, the per-timestep paste then writes windows only.  Nothing reads y_out before
      # the first paste, so the fill (134 MB at cfg2, 28 us as a launch of its own) rides on the first
      # timestep's first controller-CNN launch, which is MFMA-bound and leaves HBM idle (a side stream
      # was tried: one forked node makes the captured graph 3x slower to replay, 7.6 vs 2.45 ms pipelined)
      if self._prefill_rides(b):
        b['_fill_rider'] = True  # _run_cnn, tt == 0: the fill travels on the first controller-CNN launch
      else:
        ops.fill(b['y_out'], 1.0 / (1.0 + math.exp(5.0)))
    # the image channels' share of ctrl-CNN layer 0, b['l0cache'], is written by the first timestep's
    # own launch (its canvas is all zero, so the layer's raw sums ARE that share — _run_cnn, tt == 0)
    if 'l0cache' in b and not self.fill_cache_inline:
      ops.first_cache(b['img'], self.W['ccnn'][0][0], self.d['ccnn_channels'][1], self.d['D'], b['l0cache'])
    self._mark('pack')

  def _launch_tail(self, b, tt, want_box, src):
    d, Wt, T = self.d, self.W, self.d['T']
    H, W, Fh, Fw = d['H'], d['W'], d['Fh'], d['Fw']
    if 'ctrl_ws' in b and b.get('ctrl_batch'):
      ops.controller_batch(self.desc, src, Wt['ctrl_split'], b['h_last'][tt], b['ctrl_out'][tt], b['gmaps'][tt], b['attn'][tt],
                           b['ctrl_ws'], b['ctrl_status'], xcd_offset=b.get('ctrl_xcd_off', -1))
    elif 'ctrl_ws' in b:
      ops.controller_split(
          self.desc, src, Wt['ctrl_split'], b['h_last'][tt], b['ctrl_out'][tt], b['gmaps'][tt], b['attn'][tt],
          b['ctrl_ws'], b['ctrl_status'])
    else:
      ops.controller(self.desc, src, Wt['ctrl'], b['h_last'][tt], b['ctrl_out'][tt],
                     b['gmaps'][tt], b['attn'][tt])
    self._mark('controller')
    if want_box or self.box:
      ops.attn_box_direct(b['attn'][tt], H, W, Fh, Fw, -5.0, b['attn_box'].data_ptr() + tt * H * W * 4, T * H * W)
      if self.box:  # dense copy of this step's box for the pairwise-IoU kernel
        ops.attn_box_direct(b['attn'][tt], H, W, Fh, Fw, -5.0, b['box1'].data_ptr(), H * W)
      self._mark('attn_box')
    if self.box:
      self._box_step(b, tt)
      return
    xp = b['x_patch'][tt]
    if self.fuse_extract_conv0 and 'acnn0_plain' in Wt and self.plan['acnn'][0] == ('single', 0):
      # extract + attention-CNN layer 0 as one launch (ra_extract_conv0_f32): one link less in the tail's launch chain
      _, sc0, sh0, c0, _ = Wt['acnn'][0]
      ops.extract_conv0(b['img'], 0, b['attn'][tt], Fh, Fw, True, xp, Wt['acnn0_plain'], sc0[tt], sh0[tt], c0, True, b['acnn'][0],
                        canvas=b['canvas'], canvas_chan=d['D'])
      self._mark('extract+attn_cnn_L0')
      src = self._run_cnn(self.plan['acnn'][1:], Wt['acnn'], b['acnn'][0], b['acnn'], tt, 'attn_cnn')
    else:
      ops.extract_direct(b['img'], 0, b['attn'][tt], Fh, Fw, d['C0p'], True, xp, canvas=b['canvas'], canvas_chan=d['D'])
      self._mark('extract')
      src = self._run_cnn(self.plan['acnn'], Wt['acnn'], xp, b['acnn'], tt, 'attn_cnn')
    core = src
    L = d['acnn_nlayers']
    skips = [b['acnn'][L - 2 - k] for k in range(L - 1)] + [xp]
    for step in self.plan['adcnn']:
      if step[0] == 'pair':
        (wpa, sca, sha, ca, upa, _), (wpb, scb, shb, cb, _, _) = Wt['adcnn'][step[1]], Wt['adcnn'][step[2]]
        out = b['y_out_patch'][tt] if b['adcnn'][step[2]] is None else b['adcnn'][step[2]]
        ops.conv_pair(src, wpa, sca[tt], sha[tt], ca, wpb, scb[tt], shb[tt], cb, poolB=1,
                      upsampleA=(upa == 2), out=out)
      else:
        i = step[1]
        wp, sc, sh, cout, unpool, sidx = Wt['adcnn'][i]
        out = b['y_out_patch'][tt] if b['adcnn'][i] is None else b['adcnn'][i]
        if self.ksize['adcnn'][i] != 3:
          ops.conv2d_fused(src, wp, sc[tt], sh[tt], cout, self.ksize['adcnn'][i], relu=True, pool=1,
                           src1=None if sidx is None else skips[sidx], upsample=(unpool == 2), out=out)
        else:
          ops.conv3x3(src, wp, sc[tt], sh[tt], cout, relu=True, pool=1,
                      src1=None if sidx is None else skips[sidx], upsample=(unpool == 2), out=out)
      src = out
    self._mark('attn_dcnn')
    fused_score = self.fuse_score and self.timing is None
    if not fused_score:
      ops.dense(b['h_last'][tt], Wt['smlp_w'], Wt['smlp_b'], 'sigmoid',
                b['s_out'].data_ptr() + tt * 4, T, x1=core.view(core.shape[0], -1))
      self._mark('score')
    # y_out was prefilled with sigmoid(beta) (_launch_pack) and after the first paste the canvas
    # is >= sigmoid(beta) everywhere, so only the attention window is touched
    flags = (0 if d['disable_overwrite'] else ops.PASTE_Y_PREFILLED) | (ops.PASTE_CANVAS_FLOORED if tt > 0 else 0)
    if fused_score:  # the score MLP rides on the paste launch (one extra workgroup per image)
      ops.paste_score_direct(src, 0, b['attn'][tt], -5.0, d['disable_overwrite'],
                             b['y_out'].data_ptr() + tt * H * W * 4, T * H * W, H, W, b['canvas'], flags,
                             b['h_last'][tt], core.view(core.shape[0], -1), Wt['smlp_w'], Wt['smlp_b'],
                             b['s_out'].data_ptr() + tt * 4, T)
    else:
      ops.paste_direct(src, 0, b['attn'][tt], -5.0, d['disable_overwrite'],
                       b['y_out'].data_ptr() + tt * H * W * 4, T * H * W, H, W, canvas=b['canvas'], flags=flags)
    self._mark('paste')

  def _run_cnn(self, steps, layers, src, bufs, tt, name, plane=None, cache=None, fill=None):
    """plane: the canvas plane standing in for channel D of the FIRST layer's packed input;
    cache: the first layer's timestep-invariant image part (ops.first_cache)."""
    pc = self.d['D'] if plane is not None else -1
    ks = self.ksize['acnn'] if layers is self.W.get('acnn') else self.ksize['ccnn']  # the layers' filter sizes
    for step in steps:
      pl = plane if step[1] == 0 else None
      if step[0] == 'pair':
        (wpa, sca, sha, ca, _), (wpb, scb, shb, cb, poolb) = layers[step[1]], layers[step[2]]
        if cache is not None and pl is not None and tt == 0 and self.fill_cache_inline:
          ops.conv_pair_fill_cache(src, pl, pc, wpa, sca[tt], sha[tt], wpb, scb[tt], shb[tt], cb, cache, bufs[step[2]],
                                   fill=fill, fill_value=1.0 / (1.0 + math.exp(5.0)))
        elif cache is not None and pl is not None:
          ops.conv_pair_cached(cache, pl, pc, wpa, sca[tt], sha[tt], wpb, scb[tt], shb[tt], cb, bufs[step[2]])
        elif (self.pair_direct16 and self.pair_wino and layers is self.W.get('ccnn') and pl is None and
              ops.conv_pair16_supported(src.shape[3], ca, cb, poolb, src.shape[1], src.shape[2])):
          # K1p16: both layers direct on the bf16 matrix pipe, layer B straight from the LDS tile layer A was written to
          ops.conv_pair16(src, wpa, sca[tt], sha[tt], wpb, scb[tt], shb[tt], out=bufs[step[2]])
        elif (self.use_wino and self.pair_wino and layers is self.W.get('ccnn') and pl is None and
              self.W['ccnn_wino'][step[2]] is not None and
              ops.conv_pair_wino_supported(src.shape[3], ca, cb, poolb, src.shape[1], src.shape[2])):
          # K1pw: layer B as Winograd straight from the LDS tile layer A was written to
          ops.conv_pair_wino(src, wpa, sca[tt], sha[tt], self.W['ccnn_wino'][step[2]], scb[tt], shb[tt], out=bufs[step[2]])
        else:
          ops.conv_pair(src, wpa, sca[tt], sha[tt], ca, wpb, scb[tt], shb[tt], cb, poolB=poolb,
                        out=bufs[step[2]], plane=pl, plane_chan=pc if pl is not None else -1)
        src = bufs[step[2]]
        self._mark('%s_L%d+%d' % (name, step[1], step[2]))
      else:
        i = step[1]
        wp, sc, sh, cout, pool = layers[i]
        wino = self.W['ccnn_wino'][i] if (layers is self.W.get('ccnn') and pl is None and self.use_wino) else None
        split = None
        if self.use_split and layers is self.W.get('ccnn') and (pl is None or i == 0):
          split = self.W['ccnn_split'][i]
        elif self.use_split and layers is self.W.get('acnn'):
          split = self.W['acnn_split'][i]
        if ks[i] != 3:
          ops.conv2d_fused(src, wp, sc[tt], sh[tt], cout, ks[i], relu=True, pool=pool, out=bufs[i], plane=pl,
                           plane_chan=pc if pl is not None else -1)
        elif split is not None:
          ops.conv_split(src, split, sc[tt], sh[tt], cout, relu=True, pool=pool, out=bufs[i], plane=pl, plane_chan=pc if pl is not None else -1)
        elif wino is not None:
          ops.conv_wino(src, wino, sc[tt], sh[tt], cout, relu=True, pool=pool, out=bufs[i])
        else:
          ops.conv3x3(src, wp, sc[tt], sh[tt], cout, relu=True, pool=pool, out=bufs[i], plane=pl,
                      plane_chan=pc if pl is not None else -1)
        src = bufs[i]
        self._mark('%s_L%d' % (name, i))
    return src

  def _box_step(self, b, tt):
    """box_model.py:484-513: greedy GT match (never accumulated), canvas from noisy GT, score.
    The pixel-sized parts run in HIP (pairwise IoU of the box against the GT boxes on the streaming
    K8 kernel, the picked instance as a weighted sum); the arg-max over T values per image is
    [B,T]-sized bookkeeping."""
    d, T = self.d, self.d['T']
    box = b['box1']
    if self.box_iou_rects and 'gt_params' in b and d['W'] % 4 == 0 and T <= 32:
      # round 6: the GT boxes are filled rectangles, so the soft IoU row needs their corners, not their T planes
      # (ra_box_iou_rects_f32, the training graph's kernel): one read of the box instead of T x H x W x 4 bytes per image —
      # 63 -> 8 us per timestep at cfg3's 32 images
      iou = ops.box_iou_rects(box.view(box.shape[0], d['H'], d['W']), b['gt_params'])  # [B,T]
    else:
      iou = ops.pair_stats(box, b['box_gt'], want=('iou_soft',))['iou_soft']  # f_inter / f_union, [B,1,T]
    ops.greedy_match(iou.view(iou.shape[0], T), out=b['match'])  # matched = 0, modellib.py:365-379
    ops.weighted_sum(b['match'], b['y_gt'], b['ysel'])
    ops.canvas_max(b['canvas'].view(b['canvas'].shape + (1,)), 0, b['ysel'], b['noise'][tt])
    nsc = d['nsc']
    ops.dense(b['h_last'][tt], self.W['smlp_w'], self.W['smlp_b'],
              'sigmoid' if nsc == 1 else 'softmax', b['s_out'].data_ptr() + tt * nsc * 4,
              T * nsc)
    self._mark('box_step')

  # ------------------------------------------------------------------ public
  _prepacked = False

  def prestage_slots(self, B):
    """The buffers a pre-stage (fg_model.prestage(into=...)) writes for a batch of B: one dict per sub-batch with its packed
    input 'img' and its slices of the shared 'x' / 'd_in' / 'y_in'.  forward(x, prepacked=True) then decodes
    from them."""
    if not torch.cuda.is_available():
      raise rn.RecAttendError('the decode loop needs an MI355X (HIP device); no CPU fallback')
    device = torch.device('cuda')
    if self._stamp is None:
      self.prepare(device)
    self.alloc(B, device)
    return self.subs

  def forward(self, x, d_in=None, y_in=None, y_gt=None, noise=None, want_box=False, prepacked=False):
    """prepacked: the packed input image and the d_in / y_in buffers of prestage_slots(B) already hold this
    batch (written on the current stream); d_in / y_in are not read and the pack launch is left out."""
    if not torch.cuda.is_available():
      raise rn.RecAttendError('the decode loop needs an MI355X (HIP device); no CPU fallback')
    self._prepacked = bool(prepacked)
    device = torch.device('cuda')
    as_t = lambda a: (a if isinstance(a, torch.Tensor) else torch.from_numpy(
        np.ascontiguousarray(a, dtype=np.float32))).to(device=device, dtype=torch.float32)
    x = as_t(x)
    B = x.shape[0]
    # The weights' stamp (data pointer and version of each of ~1 400 tensors: 0.5 ms of host time at cfg2) is compared AFTER
    # the launch, while the GPU decodes: a forward that finds changed weights is prepared and launched again on the same
    # stream before anything is returned (the stale run's outputs are overwritten in stream order).  Only the first forward
    # and a forward after _stamp was reset prepare first.
    late_check = self._stamp is not None
    if not late_check:
      self.prepare(device)
    self.alloc(B, device)
    b = self.glob
    b['x'].copy_(x)
    if 'd_in' in b and not prepacked:
      b['d_in'].copy_(as_t(d_in))
    if 'y_in' in b and not prepacked:
      b['y_in'].copy_(as_t(y_in))
    if self.box:
      b['y_gt'].copy_(as_t(y_gt))
      if noise is None:
        b['noise'].uniform_(0.0, 0.3)  # box_model.py:500-502
      else:
        b['noise'].copy_(as_t(noise).reshape(b['noise'].shape))
      Bs = B // len(self.subs)
      for k, sb in enumerate(self.subs):
        sb['noise'].copy_(b['noise'][:, k * Bs:(k + 1) * Bs])
        sb['gt_params'], sb['box_gt'] = ops.gt_box(sb['y_gt'].contiguous(), float(self.d['attn_box_padding_ratio']), 10.0)
    self._last_want_box = bool(want_box)
    self._launch_forward(want_box)
    if late_check and self._weights_stamp() != self._stamp:
      self.prepare(device)  # new packed weights, graphs dropped
      self._launch_forward(want_box)
    return self

  def _launch_forward(self, want_box):
    graphable = self.use_graph and self.timing is None
    if not graphable:
      self._launch_all(want_box)
      return self
    key = (bool(want_box), True) if self._prepacked else bool(want_box)  # without a pack launch: a graph of its own
    if self.box:  # the GT boxes are a fresh tensor per forward: the graph reads a fixed buffer
      for sb in self.subs:
        if 'box_gt_buf' not in sb:
          sb['box_gt_buf'] = torch.empty_like(sb['box_gt'])
          sb['gt_params_buf'] = torch.empty_like(sb['gt_params'])
        sb['box_gt_buf'].copy_(sb['box_gt'])
        sb['box_gt'] = sb['box_gt_buf']
        sb['gt_params_buf'].copy_(sb['gt_params'])
        sb['gt_params'] = sb['gt_params_buf']
    g = self._graphs.get(key)
    if g is None:
      self._launch_all(want_box)  # warm-up (also sets kernel attributes)
      torch.cuda.synchronize()
      g = torch.cuda.CUDAGraph()
      with rn.quiet_capture(), torch.cuda.graph(g):
        self._launch_all(want_box)
      self._graphs[key] = g
    g.replay()
    return self
