/*
 * recattend.h — C ABI of librecattend.so: the MI355X (gfx950) implementation of the
 * recurrent-attention decode loop of renmengye/rec-attend-public.
 *
 * Every entry point is `extern "C"`, takes plain pointers and sizes (no torch / TF
 * types) and returns an int:
 *     0   success
 *    <0   invalid argument (RA_E_*), nothing was launched / written
 *    >0   a hipError_t raised by the runtime (see ra_last_error_string()), or for the
 *         Hungarian entry points the documented positive status 1
 * The library never allocates memory that crosses the boundary and keeps no global
 * state besides a thread-local last-error string; every buffer (inputs, outputs,
 * workspaces) is owned by the caller.  Device pointers are HIP device pointers on the
 * current device; `stream` is a hipStream_t passed as void* (NULL = default stream).
 * All tensors are float32, NHWC, densely packed unless a stride is stated.
 *
 * Reference interfaces each entry point replaces are cited as file:line of the
 * reference checkout (renmengye/rec-attend-public).
 */
#ifndef RECATTEND_H_
#define RECATTEND_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RA_E_INVALID (-1)   /* null pointer / non-positive dim */
#define RA_E_SHAPE (-2)     /* unsupported shape (alignment / divisibility) */
#define RA_E_WORKSPACE (-3) /* workspace too small */
#define RA_E_HUNG_BFS (-12)      /* hungarian.cc:124-127 LOG(FATAL) */
#define RA_E_HUNG_PATH (-13)     /* hungarian.cc:146-150,156-160 */
#define RA_E_HUNG_FLOW (-14)     /* hungarian.cc:184-188 */
#define RA_E_HUNG_EQUALIZE (-15) /* hungarian.cc:446-450 */

/* ABI version: bumped whenever an entry point of this header is removed or changes its signature (additions do not
 * bump it).  101 = round 3's removal of the table-form attention entry points and the phase-fused patch net; 102-113 =
 * rounds 3-5 (signature changes of the controller / conv entry points as the kernels were rebuilt; `git log -p
 * include/recattend.h` has each); 115 = the ragged entry points and struct ra_image_geo, an addition that was given a
 * number of its own so that a binding built for them meets a library that has them.  ra_native.py refuses a library whose
 * version differs from the header it was written against. */
#define RA_ABI_VERSION 115
int ra_version(void);
/* Human-readable description of the last non-zero return on this thread. */
const char *ra_last_error_string(void);

/* Test aid (no reference counterpart): fills the LDS of every CU with NaN, so a kernel that
 * reads shared memory it never wrote fails the parity tests deterministically. */
int ra_debug_poison_lds(void *stream);
/* Test aid (no reference counterpart): parks `n_wg` workgroups of `lds_bytes` dynamic LDS each (<= 160 KB; above 80 KB that is
 * one per CU) on XCD `xcd` (HW_REG_XCC_ID) for `millis` ms of wall clock (s_memrealtime, capped at 20 s): a launch of 8 * n_wg
 * workgroups whose members on any other XCD leave at once.  resident[0] (device int, zeroed by the caller, may be NULL) counts
 * the parked workgroups as they start.  For tests of what a launch that relies on co-residency (ra_controller_split_f32) does
 * when part of an XCD is taken: tests/test_full_model_gpu.py. */
int ra_debug_park_xcd(int xcd, int n_wg, int lds_bytes, int millis, int *resident, void *stream);

/* Test aid (no reference counterpart): the launch PLAN of a conv entry point.  The conv kernels pick their template instantiation
 * on the host from the problem size; a plan query walks the very chain of choices the launch walks (one code path: the launch
 * is that chain with plan == NULL) and, where the launch would be issued, fills plan[RA_PLAN_INTS] instead.  Nothing is
 * launched and no device memory is touched.  The RA_* tuning variables count as they do for a launch.  Fields:
 *   FAMILY   RA_PLAN_FAMILY_*: K1 = the conv3x3_mfma template (ra_conv3x3_f32 and its bf16 / moments / k x k parts), CONV8 = the
 *            entry diverts to the 8- / 16-channel full-resolution kernels (then only FORM and NC = those channels are filled)
 *   FORM     bits RA_PLAN_FORM_*: SWAP = channel-vector stores (else one value per lane), SUBPIXEL = the sub-pixel form of the
 *            stride-2 transposed conv (else zero-stuffed), BF16 = bf16 operands, MOMENTS = batch moments in the epilogue, KXK =
 *            a filter size other than 3
 *   CK, NC, WN, GX, GY, KF   the template arguments: input channels per staged chunk, cout groups per wave, waves along cout,
 *            pixel groups per wave in x / y, filter size
 *   TILE_H, TILE_W, TILES_X, TILES_Y, NTILES   a workgroup's tile, tiles per image row / column, tiles of the launch
 *   GRID, TILES_MIN, TILES_MAX   workgroups, and the fewest / most tiles one of them walks.  These need the device's CU count
 *            and the kernel's occupancy: -1 where no device can be asked (every other field is a pure function of the shape).
 *   XCD_MAP, TICKETS   1 = XCD-contiguous tile walk / tiles drawn as tickets (always 0 for K1)
 * ra_conv3x3_plan: the shape arguments of ra_conv3x3_f32 (KF = 3, all flags 0), ra_convkxk_f32 (KF), ra_conv3x3_bf16ops_f32
 * (bf16_operands), ra_conv3x3_moments_f32 (moments, with or without bf16_operands) and ra_conv3x3_bf16_f32 (bf16_operands,
 * store_flags, moments = part != NULL); has_plane: a canvas plane is given.  Returns what the launch's argument checks return. */
#define RA_PLAN_INTS 24
#define RA_PLAN_FAMILY 0
#define RA_PLAN_FORM 1
#define RA_PLAN_CK 2
#define RA_PLAN_NC 3
#define RA_PLAN_WN 4
#define RA_PLAN_GX 5
#define RA_PLAN_GY 6
#define RA_PLAN_KF 7
#define RA_PLAN_TILE_H 8
#define RA_PLAN_TILE_W 9
#define RA_PLAN_TILES_X 10
#define RA_PLAN_TILES_Y 11
#define RA_PLAN_NTILES 12
#define RA_PLAN_GRID 13
#define RA_PLAN_TILES_MIN 14
#define RA_PLAN_TILES_MAX 15
#define RA_PLAN_XCD_MAP 16
#define RA_PLAN_TICKETS 17
#define RA_PLAN_CMID 18
#define RA_PLAN_SLICES 19
#define RA_PLAN_POOL 20
#define RA_PLAN_FAMILY_K1 1
#define RA_PLAN_FAMILY_CONV8 2
#define RA_PLAN_FAMILY_PAIR 3
#define RA_PLAN_FAMILY_SPLIT 4
#define RA_PLAN_FAMILY_WINO 5
#define RA_PLAN_FAMILY_PAIR_WINO 6
#define RA_PLAN_FORM_SWAP 1
#define RA_PLAN_FORM_SUBPIXEL 2
#define RA_PLAN_FORM_BF16 4
#define RA_PLAN_FORM_MOMENTS 8
#define RA_PLAN_FORM_KXK 16
#define RA_PLAN_FORM_PERSIST 32
#define RA_PLAN_FORM_NPACKED 64
#define RA_PLAN_FORM_CACHED 128
#define RA_PLAN_FORM_SPLIT 256
#define RA_PLAN_FORM_PLANE 512
int ra_conv3x3_plan(int C0, int C1, int B, int Hs, int Ws, int upsample, int KF, int Cout, int pool, int has_plane,
                    int bf16_operands, int moments, int store_flags, int *plan);
/* The fused pair (FAMILY = PAIR): cache_form 0 = ra_conv_pair_f32 with these shape arguments, 1 = ra_conv_pair_fill_cache_f32,
 * 2 = ra_conv_pair_cached_f32 (both: B, Hs, Ws and CoutB count; the rest is fixed by the form).  CK = layer A's input channels,
 * CMID = layer A's output channels, NC = layer B's cout groups, GX / GY = layer B's pixel groups per wave (0 for the N-packed
 * kernel, which has one geometry).  FORM bits: PERSIST = conv_pair_persist_mfma (a grid of resident workgroups walking
 * tiles), NPACKED = the N-packed kernel conv_pair8_mfma, with CACHED = it reads layer A's cached partial sums and SPLIT = its
 * layer B runs the split-precision bf16 form.  TICKETS = 1: tiles are drawn as tickets where a ticket scratch is bound.  The
 * geometry and the whole N-packed plan need no device; whether the persistent kernel runs does (GRID, TILES_MIN, TILES_MAX
 * = -1 and no PERSIST bit where no device can be asked and the shape admits that kernel). */
int ra_conv_pair_plan(int Cin, int B, int Hs, int Ws, int upsampleA, int CoutA, int CoutB, int poolB, int has_plane,
                      int cache_form, int *plan);
/* K1s (FAMILY = SPLIT: ra_conv_split_f32, has_plane: ra_conv_split_plane_f32, FORM bit PLANE), Winograd (FAMILY = WINO:
 * ra_conv_wino_f32) and the Winograd pair (FAMILY = PAIR_WINO: ra_conv_pair_wino_f32; FORM bit SPLIT = layer A in the
 * split-precision bf16 form).  CK = input channels, NC = 16-channel blocks per workgroup, POOL, TILE_H (Winograd: TSY 8 or 16),
 * SLICES = grid.y, the channel slices; GRID = grid.x, the persistent workgroups that share the NTILES tiles of one slice.
 * XCD_MAP and TILES_MIN / TILES_MAX describe the static walk; TICKETS = 1: with a ticket scratch bound the tiles are drawn
 * instead.  Every one of these grids follows the device's CU count (Winograd's tile height too): RA_E_INVALID without a device. */
int ra_conv_split_plan(int B, int H, int W, int Cin, int Cout, int pool, int has_plane, int *plan);
int ra_conv_wino_plan(int B, int H, int W, int Cin, int Cout, int pool, int *plan);
int ra_conv_pair_wino_plan(int B, int H, int W, int *plan);
/* K1p16 (ra_conv_pair16_f32): FAMILY = PAIR with the FORM bits SPLIT | PERSIST, CK = 8, CMID = 16, NC = 1, POOL = 2, 8 x 16 tiles,
 * SLICES = 1; GRID, XCD_MAP, TILES_MIN / TILES_MAX and TICKETS as for the Winograd pair.  The grid follows the device's CU count
 * and the kernel's occupancy: RA_E_INVALID without a device. */
int ra_conv_pair16_plan(int B, int H, int W, int *plan);
/* Test aid (no reference counterpart): the launch plan of the direct paste (mode 0: ra_paste_direct_f32, ra_paste_score_direct_f32
 * without its rider workgroup) and of the attention box (mode 1: ra_attn_box_direct_f32; Cp, pc, has_canvas, has_img do not
 * count).  The paste launches one of two kernels on its shape and argument conditions; the query asks the launch's own
 * chooser (one host function takes these facts and returns the record the launch is made from) and fills
 * plan[RA_PASTE_PLAN_INTS] instead of launching.  has_canvas / has_img: a canvas plane / a packed image is given; aligned16: y_out, canvas and patch are all
 * 16-byte aligned.  No device is needed; RA_PASTE_GEO counts as it does for a launch.  Fields: KERNEL RA_PASTE_KERNEL_GENERAL
 * (paste_direct_kernel) or RA_PASTE_KERNEL_WINDOW (paste_win_kernel), ROWS image rows per workgroup, GRID_X (the last
 * workgroup holds H % ROWS rows where that is not 0), THREADS, LDS dynamic shared bytes.  Returns what the launch's argument
 * checks return. */
#define RA_PASTE_PLAN_INTS 8
#define RA_PASTE_PLAN_KERNEL 0
#define RA_PASTE_PLAN_ROWS 1
#define RA_PASTE_PLAN_GRID_X 2
#define RA_PASTE_PLAN_THREADS 3
#define RA_PASTE_PLAN_LDS 4
#define RA_PASTE_KERNEL_GENERAL 1
#define RA_PASTE_KERNEL_WINDOW 2
int ra_paste_plan(int mode, int B, int H, int W, int Fh, int Fw, int Cp, int pc, int has_canvas, int has_img,
                  size_t y_stride_b, int aligned16, int *plan);

/* ------------------------------------------------------------------------------------
 * Hungarian matching — replaces the TF custom op
 *   REGISTER_OP("Hungarian").Input("weights: float").Output("matching: float")
 *     .Output("cover_x: float").Output("cover_y: float")          hungarian.cc:26-30
 *   HungarianOp::Compute                                           hungarian.cc:36-85
 * weights [B,N,M] -> matching [B,N,M], cover_x [B,N] (op shape [B,N,1]), cover_y [B,M]
 * (op shape [B,1,M]).  The op's 2-D form (hungarian.cc:58-60,490-504) is B == 1.
 * Bit-exact with the reference's float32 control flow.  Returns 0, or 1 when any example
 * hit the outer 1000-iteration cap (the reference logs an error and returns the partial
 * matching, hungarian.cc:363-377 — so does this), or RA_E_HUNG_* where the reference
 * would LOG(FATAL).  Host pointers; runs on the calling thread; re-entrant.
 * ---------------------------------------------------------------------------------- */
int ra_hungarian_f32(const float *weights, int B, int N, int M, float *matching,
                     float *cover_x, float *cover_y);

/* Same contract on DEVICE pointers (one workgroup per example), so the training step
 * needs no device->host sync.  status_dev (nullable): int[B] per-example codes as above
 * (the return value only reports launch errors).  ws: device scratch of at least
 * ra_hungarian_dev_workspace_bytes(B, N, M) bytes. */
size_t ra_hungarian_dev_workspace_bytes(int B, int N, int M);
int ra_hungarian_f32_dev(const float *weights, int B, int N, int M, float *matching,
                         float *cover_x, float *cover_y, int *status_dev, void *ws,
                         size_t ws_bytes, void *stream);

/* ------------------------------------------------------------------------------------
 * K1  conv3x3 (+bias+BatchNorm(eval)+ReLU+maxpool) as an f32-MFMA implicit GEMM.
 * Replaces one layer of nnlib.cnn's run_cnn (nnlib.py:229-253: conv2d :6-12 + b,
 * batch_norm :65-128 in eval mode, act, max_pool :15-25) and — with RA_CONV_TRANSPOSED
 * packing + `upsample` — one layer of nnlib.dcnn's run_dcnn (nnlib.py:362-400:
 * concat(prev, skip), conv2d_transpose SAME stride 1|2, + b, BN, act).
 *
 * Input = channel-concat of src0 [B,Hs,Ws,C0] and (optional) src1 [B,Hs,Ws,C1];
 * C0 % 4 == 0, C1 % 4 == 0.  With upsample == 1 the conv runs over the zero-stuffed
 * image U[2i+1,2j+1] = src[i,j] of size [2Hs,2Ws] (the stride-2 transposed conv).
 * Output y [B,Ho,Wo,Cout], Ho = H/pool, Wo = W/pool, pool in {1,2} (H, W even if 2).
 * scale/shift [CoutP] fold the conv bias and BN:  y = max?(relu?(conv*scale + shift)).
 * wpacked comes from ra_conv_pack_weights (device copy of it).
 * ---------------------------------------------------------------------------------- */
#define RA_CONV_TRANSPOSED 1 /* w is a conv2d_transpose filter [3,3,Cout,Cin] (nnlib.py:320-325) */

/* Padded channel counts the kernel works in: CinP = roundup(Cin,4), CoutP in {16,32,64,128,...}. */
int ra_conv_cout_padded(int Cout);
/* Number of floats in the packed weight buffer for a [3,3,Cin,Cout] filter (Cin % 4 == 0). */
size_t ra_conv_packed_floats(int Cin, int Cout);
/* Host-side repack of a TF-layout filter into the kernel's B-operand order.
 * w: [3,3,Cin_w,Cout] (or [3,3,Cout,Cin_w] with RA_CONV_TRANSPOSED), host pointer.
 * chan_map (nullable): int[Cin] giving, for every kernel input channel, the filter's
 * input-channel index it multiplies, or -1 for a zero (padding) channel; NULL = identity
 * with Cin_w == Cin.  out: host buffer of ra_conv_packed_floats(Cin, Cout) floats. */
int ra_conv_pack_weights(const float *w, int Cin_w, int Cout, int Cin, const int *chan_map,
                         int flags, float *out);
/* Other filter sizes (nnlib.cnn / nnlib.dcnn take one per layer: nnlib.py:131-257, :260-404): KF in {1, 3, 5, 7}.
 * ra_conv_packed_floats_k: floats of the packed buffer for a [KF,KF,Cin,Cout] filter (0 for another KF or shape).
 * ra_conv_pack_weights_k: as ra_conv_pack_weights for a [KF,KF,Cin_w,Cout] (or, RA_CONV_TRANSPOSED, [KF,KF,Cout,Cin_w]:
 * flipped taps, swapped in/out) filter; packed order [chunk][tap = ky*KF+kx][cg][ksub][CoutP], channel
 * chunk*CK + 4*cg + ksub, CK = 16 / 8 / 4 (the largest dividing Cin) for KF <= 3, 8 or 4 for KF = 5, 4 for KF = 7.
 * KF = 3 is exactly ra_conv_packed_floats / ra_conv_pack_weights. */
size_t ra_conv_packed_floats_k(int KF, int Cin, int Cout);
int ra_conv_pack_weights_k(const float *w, int KF, int Cin_w, int Cout, int Cin, const int *chan_map, int flags,
                           float *out);
/* Host-side fold of bias + BN(eval) into scale/shift [CoutP] (nnlib.py:119: eps = 1e-3).
 * beta/gamma/mean/var nullable together (no BN: scale = 1, shift = bias). */
int ra_conv_fold_bn(const float *bias, const float *beta, const float *gamma, const float *mean,
                    const float *var, int Cout, float eps, float *scale, float *shift);

/* plane (nullable): a [B,Hs,Ws] tensor that REPLACES input channel plane_chan of src0 — the
 * canvas kept outside the packed image (full_model.py:648: canvas is one channel of ccnn_inp). */
int ra_conv3x3_f32(const float *src0, int C0, const float *src1, int C1, int B, int Hs, int Ws,
                   int upsample, const float *wpacked, const float *scale, const float *shift,
                   int Cout, int relu, int pool, const float *plane, int plane_chan, float *y,
                   void *stream);

/* ra_conv3x3_f32 for a KF x KF filter packed by ra_conv_pack_weights_k(KF) (nnlib.py:131-257, :260-404): SAME conv,
 * centred window; with upsample == 1 the stride-2 SAME conv2d_transpose, whose window on U is TF's asymmetric one for
 * KF = 5, 7.  Float32 operands and accumulation, same epilogue, sources and canvas plane.  KF = 3 is ra_conv3x3_f32;
 * another KF (even, or not 1 / 5 / 7) returns RA_E_SHAPE, as does a shape ra_conv3x3_f32 refuses, without a launch. */
int ra_convkxk_f32(const float *src0, int C0, const float *src1, int C1, int B, int Hs, int Ws, int upsample,
                   const float *wpacked, int KF, const float *scale, const float *shift, int Cout, int relu, int pool,
                   const float *plane, int plane_chan, float *y, void *stream);

/* K1-wide: the same fused layer for the channel widths K1 refuses — Cout 129 .. 512 (a multiple of 16), C0 + C1 <= 1024, each
 * a multiple of 4 (ra_conv_wide_supported(C0 + C1, Cout)).  These are the inner layers of fg_model, the fully
 * convolutional pre-stage that produces y_in / d_in (fg_model.py:112-160: nnlib.cnn run_cnn nnlib.py:229-253 and nnlib.dcnn
 * run_dcnn nnlib.py:362-400 with 192 .. 512 channels and skip concats of up to 1024).  Exact float32 on the f32 MFMA, both
 * operands staged through LDS, the Cout range split over workgroups in slices of 64 (csrc/ra_conv_wide.hip); no canvas
 * plane.  wpacked: ra_conv_wide_packed_floats() floats from ra_conv_wide_pack_weights (arguments as ra_conv_pack_weights;
 * packed order [co / 64][c / 16][tap][ksub][co % 64][cg], channel c = 16 chunk + 4 cg + ksub, zero past Cin and Cout).
 * scale / shift: Cout floats.  A shape outside the range returns RA_E_SHAPE without a launch. */
int ra_conv_wide_supported(int Cin, int Cout);
size_t ra_conv_wide_packed_floats(int Cin, int Cout);
int ra_conv_wide_pack_weights(const float *w, int Cin_w, int Cout, int Cin, const int *chan_map, int flags, float *out);
int ra_conv3x3_wide_f32(const float *src0, int C0, const float *src1, int C1, int B, int Hs, int Ws, int upsample,
                        const float *wpacked, const float *scale, const float *shift, int Cout, int relu, int pool,
                        float *y, void *stream);

/* The head of fg_model (fg_model.py:179-194): logits [npix, nsc + no] -> y_out [npix, nsc] = sigmoid (nsc == 1) or softmax
 * over the nsc semantic classes, d_out [npix, no] = softmax over the no orientation classes (nsc 1 .. 16; no 0 | 8, d_out
 * NULL when 0).  quantise != 0 stores floor(v * 255) / 255: the 8-bit round trip of the pack step (fg_model_pack.py:41-48
 * writes PNGs, data_api/ins_seg_dataset.py:273-292 reads them back as uint8 / 255).  packed (nullable): also writes the
 * decode loop's packed input image [npix, Cp] = [x (D) | canvas = 0 | d_out | y_out | 0 ...] — ra_pack_input_plane_f32's
 * pixel, from x [npix, D] — and zeroes canvas_plane [npix] (nullable), so a chained run needs no pack launch. */
int ra_fg_head_f32(const float *logits, size_t npix, int nsc, int no, int quantise, float *y_out, float *d_out,
                   const float *x, int D, float *packed, int Cp, float *canvas_plane, void *stream);

/* Mixed precision for the training step (model_opt['compute_dtype'] = 'bf16'; the reference trains in float32 —
 * this is an extension behind its option dictionary): the same layer with bf16 OPERANDS — pixels and weights are
 * rounded to bf16 (round-to-nearest-even) on their way from LDS / registers into v_mfma_f32_16x16x16_bf16 — and
 * float32 accumulation, epilogue and tensors. */
int ra_conv3x3_bf16ops_f32(const float *src0, int C0, const float *src1, int C1, int B, int Hs, int Ws,
                           int upsample, const float *wpacked, const float *scale, const float *shift,
                           int Cout, int relu, int pool, const float *plane, int plane_chan, float *y,
                           void *stream);

/* ---- bf16 STORAGE of the tensors between the conv layers' passes (model_opt['compute_dtype'] = 'bf16'; an extension: the
 * reference trains in float32, full_model.py:1039-1057).  On top of the bf16-operand kernels above, the pre-activation
 * outputs U, the activations Y and the gradients dY / dU are kept as bf16 in HBM (2 bytes per element, round to nearest
 * even on the way out, exact on the way in); BatchNorm statistics, sums, parameter gradients, master weights and Adam
 * state stay float32.  Tensors in bf16 are `void *`. ---- */
/* conv3x3 with bf16 operands; store_flags bit 0: src0 / src1 hold bf16, bit 1: y is written as bf16.  part != NULL: the
 * batch moments of the float32 accumulators as ra_conv3x3_moments_f32 (pool 1, Cout % 4 == 0); part == NULL: `pool` as given. */
int ra_conv3x3_bf16_f32(const void *src0, int C0, const void *src1, int C1, int B, int Hs, int Ws, int upsample,
                        const float *wpacked, const float *scale, const float *shift, int Cout, int relu, int pool, void *y,
                        float *part, size_t part_floats, int *nparts, int store_flags, void *stream);
/* ra_bn_act_pool_f32 with flags bit 0: u stored as bf16, bit 1: y written as bf16 (0, 1, 3; C % 4 == 0, C / 4 a power of two). */
int ra_bn_act_pool_bf16_f32(const void *u, const float *mean, const float *var, const float *gamma, const float *beta, float eps,
                            int relu, int pool, int B, int H, int W, int C, void *y, int flags, void *stream);
/* ra_bn_act_pool_bwd_acc_f32 / ra_bn_act_pool_bwd_grouped_f32 with flags bit 0: u read and du written as bf16, bit 1: dy read
 * as bf16 (0, 1, 3). */
int ra_bn_act_pool_bwd_acc_bf16_f32(const void *u, const void *dy, const float *mean, const float *var, const float *gamma,
                                    const float *beta, float eps, int relu, int pool, int B, int H, int W, int C, float *ws,
                                    size_t ws_floats, float *dgamma, float *dbeta, void *du, float *acc_gamma, float *acc_beta,
                                    int flags, void *stream);
int ra_bn_act_pool_bwd_grouped_bf16_f32(const void *u, const void *dy, const void *const *tabs, int G, float eps, int relu, int pool,
                                        int B, int H, int W, int C, float *ws, size_t ws_floats, float *dgamma, float *dbeta,
                                        void *du, int flags, void *stream);
/* ra_conv3x3_wgrad_acc_bf16ops_f32 with fmt bit 0: x stored as bf16, bit 1: du stored as bf16.  (The multi-call form
 * ra_conv3x3_wgrad_multi_acc_f32 takes the same two bits shifted up by one in its bf16_operands argument.) */
int ra_conv3x3_wgrad_acc_bf16_f32(const void *x, int Cin, int B, int Hs, int Ws, int upsample, const void *du, int Cout, float *ws,
                                  size_t ws_floats, const int *chan_map, int cin_w, int transposed, float *gw, float *gb, int fmt,
                                  void *stream);

/* The training forward of a BatchNorm layer (nnlib.py:98: tf.nn.moments of the conv output over batch, height, width):
 * ra_conv3x3_moments_f32 is ra_conv3x3_f32 / _bf16ops_f32 (pool 1, Cout % 4 == 0, no canvas plane) whose epilogue also
 * leaves per-wave channel sums of its output y BEFORE the ReLU in `part` (ra_conv3x3_moments_part_floats(Cout) floats;
 * *nparts = records written, a host int); ra_bn_moments_from_partials_f32 combines them (Chan's update, float64) into
 * mean[C] / var[C] (biased, as tf.nn.moments).  One small launch instead of two more passes over y. */
size_t ra_conv3x3_moments_part_floats(int Cout);
int ra_conv3x3_moments_f32(const float *src0, int C0, const float *src1, int C1, int B, int Hs, int Ws,
                           int upsample, const float *wpacked, const float *scale, const float *shift,
                           int Cout, int relu, int bf16_operands, float *y, float *part, size_t part_floats,
                           int *nparts, void *stream);
int ra_bn_moments_from_partials_f32(const float *part, int nparts, int C, float *mean, float *var, void *stream);

/* Two consecutive layers fused in one launch (the intermediate activation stays in LDS):
 *   A: conv3x3 + scale/shift [+ReLU], no pool, optional zero-stuffed (stride-2 transposed) input
 *   B: conv3x3 + scale/shift [+ReLU] + max-pool poolB
 * src [B,Hs,Ws,Cin] single source, Cin in {4,8,16,32}; CoutA in {8,16,32}; CoutB <= 32.
 * wpA / wpB from ra_conv_pack_weights with Cin resp. CoutA input channels. */
int ra_conv_pair_supported(int Cin, int CoutA, int CoutB);
int ra_conv_pair_f32(const float *src, int Cin, int B, int Hs, int Ws, int upsampleA,
                     const float *wpA, const float *scaleA, const float *shiftA, int CoutA, int reluA,
                     const float *wpB, const float *scaleB, const float *shiftB, int CoutB, int reluB,
                     int poolB, const float *plane, int plane_chan, float *y, void *stream);

/* K1s (round 5) — the same layer (conv3x3 SAME + folded BatchNorm + ReLU + max-pool, nnlib.py:229-253) as a DIRECT convolution
 * on the BF16 matrix pipe at float32 accuracy: every float32 operand is the exact sum of three bf16 pieces, and six of the
 * nine piece products (everything above 2^-24 of a product) run as v_mfma_f32_16x16x32_bf16 with float32 accumulation
 * (csrc/ra_conv_split.hip).  Cin in {16, 24, 32, 64}, Cout % 16 == 0, pool 1 | 2, H and W multiples of 4 (round 6: the 16 x 16
 * tiles — 8 rows at Cin = 64 — may be ragged at the right and bottom edges: KITTI's 56- and 28-pixel maps, the 24- and 12-pixel
 * patch maps) (ra_conv_split_supported).  wpacked: ra_conv_split_packed_halfs() 16-bit words, the filter's three bf16 pieces in B-operand
 * order, from the reference's [3,3,Cin,Cout] filter by ra_conv_split_pack_weights (host) or ra_conv_split_pack_weights_dev
 * (device pointers; transposed != 0: w is a conv2d_transpose filter [3,3,Cout,Cin] — taps flipped, in / out swapped, as
 * RA_CONV_TRANSPOSED: the packing of a cnn layer's DATA GRADIENT, which the training step runs as this conv with scale 1,
 * shift 0).  scale / shift as ra_conv3x3_f32. */
int ra_conv_split_supported(int Cin, int Cout, int pool, int H, int W);
size_t ra_conv_split_packed_halfs(int Cin, int Cout);
int ra_conv_split_pack_weights(const float *w, int Cin, int Cout, unsigned short *out);
int ra_conv_split_pack_weights_dev(const float *w, int Cin, int Cout, int transposed, unsigned short *out, void *stream);
int ra_conv_split_f32(const float *x, int B, int H, int W, int Cin, const unsigned short *wpacked, const float *scale,
                      const float *shift, int Cout, int relu, int pool, float *y, void *stream);
/* ... with channel plane_chan of x taken from the plane [B,H,W] instead (round 6; Cin 16 | 24 | 32): the FIRST controller-CNN
 * layer of the KITTI / Cityscapes architectures, whose packed input concat(x, canvas, d_in, y_in) (full_model.py:640-661; 13 / 21
 * channels packed to 16 / 24) keeps the canvas in its own plane (as ra_conv3x3_f32's plane / plane_chan). */
int ra_conv_split_plane_f32(const float *x, int B, int H, int W, int Cin, const float *plane, int plane_chan,
                            const unsigned short *wpacked, const float *scale, const float *shift, int Cout, int relu, int pool,
                            float *y, void *stream);

/* K1w: conv3x3 SAME + folded BN + ReLU + optional 2x2 max-pool (nnlib.py:229-253) as Winograd F(2x2, 3x3)
 * on the f32 MFMA: 2.25x fewer matrix multiplies than ra_conv3x3_f32 for the same layer, results equal
 * to ~1e-6 relative (summation order and the 0.5 factors of the filter transform).  Cin 16 | 32,
 * Cout % 16 == 0, H and W multiples of 16 (ra_conv_wino_supported).  wpacked: the transformed filters
 * G g G^T in MFMA B-operand order, ra_conv_wino_packed_floats() floats, from the reference's
 * [3,3,Cin,Cout] filter by ra_conv_wino_pack_weights (host).  scale / shift: the folded BatchNorm of
 * this timestep, as for ra_conv3x3_f32.  x [B,H,W,Cin] -> y [B,H/pool,W/pool,Cout]. */
int ra_conv_wino_supported(int Cin, int Cout, int pool, int H, int W);
size_t ra_conv_wino_packed_floats(int Cin, int Cout);
int ra_conv_wino_pack_weights(const float *w, int Cin, int Cout, float *out);
int ra_conv_wino_f32(const float *x, int B, int H, int W, int Cin, const float *wpacked,
                     const float *scale, const float *shift, int Cout, int relu, int pool, float *y,
                     void *stream);

/* K1pw: ra_conv_pair_f32 for the pair 8 -> 16 -> 16 with poolB = 2 (the controller CNN's L2+L3 at the CVPPP
 * arch, full_model.py:640-661 / nnlib.py:229-253) with layer B computed as Winograd F(2x2,3x3) straight
 * from the LDS tile layer A was written to.  wpA: ra_conv_pack_weights (Cin = 8); wpB_wino:
 * ra_conv_wino_pack_weights of layer B's [3,3,16,16] filter.  H, W multiples of 16. */
int ra_conv_pair_wino_supported(int Cin, int CoutA, int CoutB, int poolB, int H, int W);
int ra_conv_pair_wino_f32(const float *x, int B, int H, int W, const float *wpA, const float *scaleA,
                          const float *shiftA, int reluA, const float *wpB_wino, const float *scaleB,
                          const float *shiftB, int reluB, float *y, void *stream);

/* K1p16: the same pair (8 -> 16 -> 16, poolB = 2; H, W multiples of 16: ra_conv_pair16_supported is the predicate of
 * ra_conv_pair_wino_supported) with BOTH layers direct on the bf16 matrix pipe at float32 accuracy (three bf16 pieces per
 * operand, six piece products per K = 32 block, as K1s): layer B reads layer A's output from LDS as bf16 pieces, a lane's four
 * accumulator registers are one pool window, and there is no Winograd transform or exchange (csrc/ra_conv_pair16.hip).  wpA and
 * wpB: ra_conv_pack_weights with Cin = 8 resp. 16, the packing ra_conv_pair_f32 takes.  Results differ from ra_conv_pair_wino_f32
 * by float32 rounding only. */
int ra_conv_pair16_supported(int Cin, int CoutA, int CoutB, int poolB, int H, int W);
int ra_conv_pair16_f32(const float *x, int B, int H, int W, const float *wpA, const float *scaleA, const float *shiftA,
                       int reluA, const float *wpB, const float *scaleB, const float *shiftB, int reluB, float *y,
                       void *stream);

/* The first controller-CNN pair with the image part of layer A cached.  Of layer A's input
 * concat(x, canvas) (full_model.py:640-661) only the canvas changes between timesteps
 * (:843-848), and a convolution is linear in its input channels, so
 *   S = sum_{taps, ci != plane_chan} x * W          (no bias, no BN)
 * is computed ONCE per forward (ra_conv_first_cache_f32; `cache` holds it in the accumulator
 * layout of the pair kernel, ra_conv_first_cache_floats() floats) and every timestep computes
 *   A = relu?((S + conv(canvas, W[:, :, plane_chan, :])) * scaleA(tt) + shiftA(tt)),  B as in
 * ra_conv_pair_f32 with poolB = 2 — 3 instead of 12 MFMA k-steps for layer A and 4 instead of 20
 * staged bytes per pixel.  Cin = 4, CoutA = 8, CoutB <= 8 only (ra_conv_first_cache_supported);
 * src [B,H,W,4] packed image, plane [B,H,W] the canvas, wpA packed for Cin = 4. */
int ra_conv_first_cache_supported(int Cin, int CoutA, int CoutB, int poolB, int H, int W);
size_t ra_conv_first_cache_floats(int B, int H, int W);
int ra_conv_first_cache_f32(const float *src, int B, int H, int W, const float *wpA, int CoutA,
                            int plane_chan, float *cache, void *stream);
/* The first timestep of a forward, where the canvas is all zero (full_model.py:239): the plain pair
 * (layer A over all 4 channels) that also WRITES the cache — with a zero canvas layer A's raw sums are
 * exactly the image part — so that no separate cache launch is needed.  The caller must only use it
 * while `plane` is zero. */
int ra_conv_pair_fill_cache_f32(const float *src, const float *plane, int plane_chan, int B, int H,
                                int W, const float *wpA, const float *scaleA, const float *shiftA,
                                int reluA, const float *wpB, const float *scaleB,
                                const float *shiftB, int CoutB, int reluB, float *cache, float *y,
                                void *stream);
/* The same launch with a constant fill riding on it: fill_dst[0 .. fill_floats) = fill_value, written a few
 * stores per thread and tile by the workgroups of this (MFMA-bound) kernel while HBM is otherwise idle.  The
 * decode loop's once-per-forward prefill of y_out (sigmoid(beta) outside every attention window,
 * full_model.py:813-818) travels this way instead of as a 28 us launch of its own.  fill_dst 16-byte
 * aligned, fill_floats % 4 == 0, < 2 GiB; fill_dst == NULL: no fill. */
int ra_conv_pair_fill_cache_rider_f32(const float *src, const float *plane, int plane_chan, int B, int H, int W,
                                      const float *wpA, const float *scaleA, const float *shiftA, int reluA,
                                      const float *wpB, const float *scaleB, const float *shiftB, int CoutB,
                                      int reluB, float *cache, float *y, float *fill_dst, size_t fill_floats,
                                      float fill_value, void *stream);
int ra_conv_pair_cached_f32(const float *cache, const float *plane, int plane_chan, int B, int H,
                            int W, const float *wpA, const float *scaleA, const float *shiftA,
                            int reluA, const float *wpB, const float *scaleB, const float *shiftB,
                            int CoutB, int reluB, float *y, void *stream);

/* ------------------------------------------------------------------------------------
 * K2  controller: glimpse read-out + LSTM + glimpse MLP (x iters) + controller MLP +
 * attention-parameter decode.  Replaces full_model.py:668-722 (= box_model.py:416-468):
 * nnlib.lstm unroll (nnlib.py:637-649, state = [c|h], zeroed every call
 * full_model.py:674), nnlib.mlp run_mlp (nnlib.py:476-493) for glimpse_mlp (relu..,
 * softmax) and ctrl_mlp, modellib.get_unnormalized_attn (modellib.py:843-847),
 * get_normalized_var (:782-793).
 * One workgroup per example.
 * ---------------------------------------------------------------------------------- */
typedef struct ra_ctrl_desc {
  int G;        /* glimpse map size gh*gw (full_model.py:311) */
  int Cf;       /* feature depth (full_model.py:312), % 4 == 0 */
  int hid;      /* ctrl_rnn_hid_dim, % 4 == 0, <= 256 */
  int iters;    /* num_ctrl_rnn_iter */
  int n_gmlp;   /* num_glimpse_mlp_layers (>= 1); dims hid,..,hid,G */
  int n_cmlp;   /* num_ctrl_mlp_layers (>= 1); dims hid, mlp_dim.., 9 */
  int mlp_dim;  /* ctrl_mlp_dim, % 4 == 0 */
  int H, W;     /* image size, for the un-normalisation */
  int Fh, Fw;   /* filter (patch) size */
  int squash;       /* squash_ctrl_params (full_model.py:695-697) */
  int fixed_var;    /* full_model.py:702-706 */
  int dynamic_var;  /* full_model.py:708-709 */
  int fixed_gamma;  /* full_model.py:711-716 */
} ra_ctrl_desc;

/* Packed controller weights (device), produced on the host by ra_ctrl_pack_weights:
 *   lstm  [(Cf+hid)][4*hid]   rows = [x ; h], columns gate-major i,f,o,u ; + bias [4*hid]
 *   gmlp  layer l: [hid][NoutP_l] + bias[NoutP_l]   (last layer NoutP = roundup(G,4))
 *   cmlp  layer l: [..][NoutP_l] + bias            (last layer 9 -> 12)
 * Layout offsets are internal; both sides use ra_ctrl_packed_floats. */
size_t ra_ctrl_packed_floats(const ra_ctrl_desc *d);
/* lstm_w: 12 host pointers in the order w_xi,w_hi,b_i, w_xf,w_hf,b_f, w_xu,w_hu,b_u,
 * w_xo,w_ho,b_o (nnlib.py:532-609); gmlp_w / cmlp_w: {w_0,b_0,w_1,b_1,...}. */
int ra_ctrl_pack_weights(const ra_ctrl_desc *d, const float *const *lstm_w,
                         const float *const *gmlp_w, const float *const *cmlp_w, float *out);

#define RA_ATTN_STRIDE 16
/* attn record [B][RA_ATTN_STRIDE]: 0 ctr_y, 1 ctr_x, 2 size_y, 3 size_x, 4 lg_var_y,
 * 5 lg_var_x, 6 attn_gamma = exp(lg_gamma), 7 box_gamma = exp(box_lg_gamma),
 * 8 y_out_lg_gamma, 9 ctr_norm_y, 10 ctr_norm_x, 11 lg_size_y, 12 lg_size_x. */
int ra_controller_f32(const ra_ctrl_desc *d, const float *feat /*[B,G,Cf]*/, const float *wpacked,
                      int B, float *h_last /*[B,hid]*/, float *ctrl_out /*[B,9]*/,
                      float *glimpse_maps /*[B,iters,G] nullable*/,
                      float *attn /*[B,RA_ATTN_STRIDE]*/, void *stream);

/* Split form of the same controller: 16 workgroups per example, each keeping its slice of
 * the LSTM / glimpse-MLP weights in LDS for the whole launch and exchanging only the small
 * activation vectors through 8-byte {tag, value} granules in `ws` (device, must be zero-filled
 * ONCE when allocated; generation-tagged, so graph replays need no memset; one workspace per
 * concurrently running launch).  Same results up to float32 summation order.  B <= 14.
 * status_dev (nullable): set to 1 if a peer workgroup timed out.  * Round 5: where the device's workgroups report the XCC ids 0..7, the launch is a 1-D grid whose workgroups draw their (image,
 * slice) role from a per-XCD ticket (behind the images' granules in `ws`: ra_ctrl_split_workspace_bytes includes it), so that
 * the 16 workgroups of an image share ONE XCD's L2 and exchange through plain stores and L1-bypassing loads instead of
 * agent-scope atomics: 63 -> 57 us per launch at cfg2.  RA_CTRL_XCD=0 selects the grid (16, B) form.  Same results bit for bit.
*/
int ra_ctrl_split_supported(const ra_ctrl_desc *d);
size_t ra_ctrl_split_packed_floats(const ra_ctrl_desc *d);
size_t ra_ctrl_split_workspace_bytes(const ra_ctrl_desc *d, int B);
int ra_ctrl_split_pack_weights(const ra_ctrl_desc *d, const float *const *lstm_w,
                               const float *const *gmlp_w, const float *const *cmlp_w, float *out);
int ra_controller_split_f32(const ra_ctrl_desc *d, const float *feat, const float *wpacked, int B,
                            float *h_last, float *ctrl_out, float *glimpse_maps, float *attn,
                            void *ws, size_t ws_bytes, int *status_dev, void *stream);
/* K2b: the split controller with its 16 weight slices shared by groups of g = ra_ctrl_batch_group_images(d, B)
 * images — 4 for launches of up to 8 images, 8 above where that fits the LDS — (16 workgroups per GROUP
 * instead of per image; weights packed exactly as for ra_controller_split_f32).  Results equal ra_controller_split_f32's to float32 round-off; a launch is
 * ceil(B / g) * 16 workgroups (at most 224: RA_E_SHAPE beyond), so several
 * launches from different streams are resident together (ra_controller_split_f32 beside its own kind
 * can starve: its spinning workgroups hold the CUs their peers wait for).  ws: zero-filled,
 * ra_ctrl_batch_workspace_bytes(), owned by one stream of launches; status_dev as above. */
int ra_ctrl_batch_group_images(const ra_ctrl_desc *d, int B);
int ra_ctrl_batch_supported(const ra_ctrl_desc *d);
size_t ra_ctrl_batch_workspace_bytes(const ra_ctrl_desc *d, int B);
int ra_controller_batch_f32(const ra_ctrl_desc *d, const float *feat, const float *wpacked, int B,
                            float *h_last, float *ctrl_out, float *glimpse_maps, float *attn, void *ws,
                            size_t ws_bytes, int *status_dev, void *stream);
/* ... on the XCD-local exchange (round 6): group g's 16 workgroups run on XCD (g + xcd_offset) mod 8 and exchange through that XCD's
 * L2 (as ra_controller_split_f32's XCD-local form) instead of agent-scope atomics.  At most 8 groups per launch; the CALLER vouches that
 * launches which can run at the same time use offsets that keep their groups on different XCDs (DecodePipeline: slot k of 4 streams with 2
 * groups each -> offset 2 k).  xcd_offset < 0, more than 8 groups, RA_CTRL_XCD=0 or a device whose workgroups do not report XCC ids 0..7:
 * the agent-scope form (= ra_controller_batch_f32).  Same workspace (ra_ctrl_batch_workspace_bytes holds the role tickets). */
int ra_controller_batch_xcd_f32(const ra_ctrl_desc *d, const float *feat, const float *wpacked, int B,
                                float *h_last, float *ctrl_out, float *glimpse_maps, float *attn, void *ws,
                                size_t ws_bytes, int *status_dev, int xcd_offset, void *stream);

/* ------------------------------------------------------------------------------------
 * K3/K5  Gaussian attention.  Replaces modellib.get_gaussian_filter (modellib.py:581-612),
 * modellib.extract_patch (modellib.py:615-641) and their uses full_model.py:778-789
 * (read) and :810-818,:843-845 (write + canvas), :738-741 (attention box).
 * ---------------------------------------------------------------------------------- */
/* Dense filter bank, the literal operator: out[b,l,f] (modellib.py:610-611). */
int ra_gaussian_filter_f32(const float *center, const float *size, const float *lg_var, int B,
                           int L, int F, float *out, void *stream);

/* The attention resample of the decode loop (K3 extract, K5 paste, the attention box).  The filter weights
 * (modellib.get_gaussian_filter, modellib.py:581-612) are evaluated on the fly from the attention records: no
 * [L,F] tables; terms below e^-30 of a tap's peak are dropped.  The canvas may live in its own plane `canvas`
 * [B,H,W] (then channel canvas_chan of img is ignored / untouched); with canvas == NULL it is channel canvas_chan
 * of img.
 *   extract (modellib.extract_patch :615-641, full_model.py:788-789):
 *     patch[b,j,i,c] = attn_gamma_b * sum_{l,w} fy[b,l,j] * img[b,l,w,chan0+c] * fx[b,w,i]
 *     img [B,H,W,Ci] (Ci % 4 == 0), patch [B,Fh,Fw,Cp] (Cp % 4 == 0, Cp <= Ci - chan0, chan0 % 4 == 0);
 *     use_gamma = 0 skips the attn_gamma factor.
 *   paste (full_model.py:810-818,843-845):
 *     y = sigmoid(exp(y_out_lg_gamma) * (fy P fx^T) + beta);  if disable_overwrite: y *= (1 - canvas);
 *     y_out[b] = y;  canvas = max(canvas, y).  P = patch[b,:,:,pc] with channel stride Cp; y_out points at the
 *     [H,W] plane of example 0 and y_stride_b floats separate examples (a [B,T,H,W] tensor is written in place,
 *     full_model.py:855).
 *   box (full_model.py:738-741, box_model.py:479-482): box = sigmoid(box_gamma * (fy 1 fx^T) + beta). */
int ra_extract_direct_f32(const float *img, int Ci, int chan0, const float *canvas, int canvas_chan,
                          const float *attn, int B, int H, int W, int Fh, int Fw, int Cp,
                          int use_gamma, float *patch, void *stream);
/* extract + layer 0 of the attention CNN in ONE launch (full_model.py:788-795; nnlib.py:229-253 for a 3x3 layer without
 * pooling): x_patch as ra_extract_direct_f32 writes it AND y0[b,j,i,co] = relu?((sum_{ky,kx,c} w0[ky][kx][c][co] *
 * x_patch[b, j+ky-1, i+kx-1, c]) * scale[co] + shift[co]) (SAME padding; scale / shift = the folded bias + BatchNorm(eval)
 * of ra_conv_fold_bn).  w0: the layer's filter in the PACKED input's channel order, [3][3][4][Cout] floats (rows of input
 * channels the model does not feed are zero).  Workgroup (tap j, image) reduces the rows of taps j-1, j, j+1 once — their
 * bands overlap almost completely — so the conv costs no second launch and no cross-workgroup wait.  Shapes:
 * ra_extract_conv0_supported (one packed channel group Cp = 4, Fw <= 64, Cout <= 16, pool 1). */
int ra_extract_conv0_supported(int Cp, int Fh, int Fw, int Cout, int pool);
int ra_extract_conv0_f32(const float *img, int Ci, int chan0, const float *canvas, int canvas_chan,
                         const float *attn_rec, int B, int H, int W, int Fh, int Fw, int use_gamma, float *patch,
                         const float *w0, const float *scale, const float *shift, int Cout, int relu, float *y0,
                         void *stream);
/* flags (promises by the caller that let the paste touch only the attention window):
 *   RA_PASTE_Y_PREFILLED     y_out already holds sigmoid(beta) everywhere (ignored with
 *                            disable_overwrite, where untouched pixels are sigmoid(beta)*(1-canvas))
 *   RA_PASTE_CANVAS_FLOORED  canvas >= sigmoid(beta) everywhere already (true after the first
 *                            paste of a sequence that started from canvas = 0) */
#define RA_PASTE_Y_PREFILLED 1
#define RA_PASTE_CANVAS_FLOORED 2
int ra_paste_direct_f32(const float *patch, int Cp, int pc, const float *attn, int B, int H, int W,
                        int Fh, int Fw, float beta, int disable_overwrite, float *canvas, float *img,
                        int Ci, int canvas_chan, float *y_out, size_t y_stride_b, int flags,
                        void *stream);
/* ra_paste_direct_f32 on a canvas plane, with the score MLP of the same timestep
 * (full_model.py:794,821-822: s = sigmoid([h | h_core] . w + bias), h [B,K0], core [B,K1],
 * w [K0+K1], bias [1]) riding along as one extra workgroup per image: s_out[b * s_stride_b]. */
int ra_paste_score_direct_f32(const float *patch, int Cp, int pc, const float *attn, int B, int H,
                              int W, int Fh, int Fw, float beta, int disable_overwrite,
                              float *canvas, float *y_out, size_t y_stride_b, int flags,
                              const float *h, int K0, const float *core, int K1, const float *w,
                              const float *bias, float *s_out, size_t s_stride_b, void *stream);

/* Adjoints of the attention resample for the training step (ra_train.AttnExtract / AttnPaste), without the dense
 * [L,F] filter banks the reference differentiates through (modellib.py:581-641): with E(X) = fy^T X fx,
 *   RA_RESAMPLE_READ   x_patch = gamma E(img) (full_model.py:788-789): X = img [B,H,W,Cx] channels chan0 .. chan0+C,
 *                      Q = d x_patch [B,Fh,Fw,Cq]; scale = gamma [B]: out[:, 0:6] are multiplied by it;
 *                      out[:, 6] = sum E.Q = d gamma.
 *   RA_RESAMPLE_WRITE  y = sigmoid(exp(rec[8]) fy P fx^T + beta) (full_model.py:810-818): dY, Y [B,H,W] (the upstream
 *                      gradient and the forward's result), Q = P [B,Fh,Fw,Cq] channel 0; E [B,Fh,Fw,Ce] channel 0
 *                      receives dP; out[:, 6] = d y_lg_gamma.
 *   RA_RESAMPLE_BOX    box = sigmoid(rec[7] fy 1 fx^T + beta) (full_model.py:738-741): Q = NULL; div = box_gamma [B]:
 *                      out[:, 6] = d box_gamma.
 * out [B,8] = (d ctr_y, d ctr_x, d size_y, d size_x, d lg_var_y, d lg_var_x, the gamma gradient, 0) for the window
 * parameters of attn_rec [B,RA_ATTN_STRIDE].  ws: ra_resample_bwd_workspace_floats(B, Fh, C) floats (C = 1 for WRITE /
 * BOX).  Deterministic (fixed-order sums); banded like the forward kernels (weights below e^-30 of the peak dropped). */
#define RA_RESAMPLE_READ 0
#define RA_RESAMPLE_WRITE 1
#define RA_RESAMPLE_BOX 2
/* The controller of the training graph (full_model.py:668-689) as one forward and one backward launch per timestep
 * (ra_train.ControllerFn): feat [B,G,Cf]; Wg [Cf+hid, 4 hid] = the LSTM's [w_x ; w_h] with the gates side by side in the
 * order i f o u (nnlib.py:641-646), bg [4 hid]; W0 [hid,hid], W1 [hid,G] the two glimpse-MLP layers (ReLU, softmax over
 * the feature map); Wc [hid,nout] the one-layer controller MLP.  The forward writes h_last [B,hid], co [B,nout] and
 * `save` (B * ra_ctrl_train_save_floats floats: per iteration xh | gates | c | z1 | map).  The backward takes d h_last /
 * d co (either may be NULL), writes d feat [B,G,Cf] and the pre-activation gradients dpre [B,iters,4 hid], dz1
 * [B,iters,hid], dlog [B,iters,G]; the parameter gradients are the caller's GEMMs of the saved layer inputs against
 * them (one per weight per optimisation step).  ra_ctrl_train_supported: LDS / thread-count limits of the kernels. */
int ra_ctrl_train_supported(int G, int Cf, int hid, int iters, int nout);
size_t ra_ctrl_train_save_floats(int G, int Cf, int hid, int iters);
int ra_ctrl_train_fwd_f32(int B, int G, int Cf, int hid, int iters, int nout, const float *feat, const float *Wg,
                          const float *bg, const float *W0, const float *b0, const float *W1, const float *b1,
                          const float *Wc, const float *bc, float *h_last, float *co, float *save, void *stream);
int ra_ctrl_train_bwd_f32(int B, int G, int Cf, int hid, int iters, int nout, const float *feat, const float *Wg,
                          const float *W0, const float *W1, const float *Wc, const float *save, const float *dh_last,
                          const float *dco, float *dfeat, float *dpre, float *dz1, float *dlog, void *stream);
/* The same for any depth of the two MLPs (full_model.py:350-352,382-384; up to 4 layers each): the glimpse MLP is n_glimpse
 * layers [hid] * n_glimpse + [G] (ReLU on all but the last), the controller MLP n_ctrl layers [hid] + [mlp_dim] * (n_ctrl - 1) +
 * [nout].  gW / gb / cW / cb: HOST arrays of device pointers, one per layer.  save: B * ra_ctrl_train_save_floats_n floats
 * (per iteration xh | gates | c | the glimpse MLP's (n_glimpse - 1) hidden layers | map); save_c [B, (n_ctrl - 1) mlp_dim]: the
 * controller MLP's hidden layers (NULL for one layer).  The backward writes the pre-activation gradients of every dense
 * layer: dpre, dlog as above, dzg = (n_glimpse - 1) layers of [B, iters, hid] dzg_stride floats apart, dzc = (n_ctrl - 1)
 * layers of [B, mlp_dim] dzc_stride apart. */
int ra_ctrl_train_supported_n(int G, int Cf, int hid, int iters, int nout, int n_glimpse, int n_ctrl, int mlp_dim);
size_t ra_ctrl_train_save_floats_n(int G, int Cf, int hid, int iters, int n_glimpse);
int ra_ctrl_train_fwd_n_f32(int B, int G, int Cf, int hid, int iters, int nout, int n_glimpse, int n_ctrl, int mlp_dim,
                            const float *feat, const float *Wg, const float *bg, const float *const *gW,
                            const float *const *gb, const float *const *cW, const float *const *cb, float *h_last,
                            float *co, float *save, float *save_c, void *stream);
int ra_ctrl_train_bwd_n_f32(int B, int G, int Cf, int hid, int iters, int nout, int n_glimpse, int n_ctrl, int mlp_dim,
                            const float *feat, const float *Wg, const float *const *gW, const float *const *cW,
                            const float *save, const float *save_c, const float *dh_last, const float *dco, float *dfeat,
                            float *dpre, float *dlog, float *dzg, size_t dzg_stride, float *dzc, size_t dzc_stride,
                            void *stream);

size_t ra_resample_bwd_workspace_floats(int B, int Fh, int C);
int ra_resample_bwd_f32(int mode, const float *X, int Cx, int chan0, int C, const float *dY, const float *Y,
                        const float *attn_rec, const float *Q, int Cq, float *E, int Ce, int B, int H, int W, int Fh,
                        int Fw, const float *scale, int scale_stride, const float *div, int div_stride, float *ws,
                        size_t ws_floats, float *out, void *stream);
int ra_attn_box_direct_f32(const float *attn, int B, int H, int W, int Fh, int Fw, float beta,
                           float *box_out, size_t stride_b, void *stream);

/* Generic dense extract_patch with caller-supplied filters (the operator surface of
 * modellib.extract_patch for arbitrary f_y [B,H,FH], f_x [B,W,FW]; x [B,H,W,D]). */
int ra_extract_patch_dense_f32(const float *x, const float *f_y, const float *f_x, int B, int H,
                               int W, int D, int FH, int FW, float *out, void *stream);

/* ------------------------------------------------------------------------------------
 * K6  small dense layers (nnlib.mlp run_mlp, nnlib.py:476-493): out = act(x W + b).
 * x = concat(x0 [B,K0], x1 [B,K1]) (x1 nullable) — the score MLP's
 * concat([h_crnn, h_core]) of full_model.py:821-822.  W [K0+K1, N] row-major.
 * act: 0 none, 1 relu, 2 sigmoid, 3 softmax (over N), 4 tanh.
 * ---------------------------------------------------------------------------------- */
int ra_dense_f32(const float *x0, int K0, const float *x1, int K1, const float *W, const float *b,
                 int B, int N, int act, float *out, size_t out_stride_b, void *stream);

/* Elementwise helpers on the path. */
/* packed[b,h,w,:] = [x (D) | canvas=0 | d_in (Dd) | y_in (Dy) | zero pad] -> Cp channels
 * (full_model.py:239,640-661; the canvas lives as channel D of the packed image). */
int ra_pack_input_f32(const float *x, int D, const float *d_in, int Dd, const float *y_in, int Dy,
                      int B, int H, int W, int Cp, float *packed, void *stream);
/* ... and, in the same pass, zeroes the decode loop's separate canvas plane [B,H,W] (canvas_plane may be
 * NULL): one launch less per forward. */
int ra_pack_input_plane_f32(const float *x, int D, const float *d_in, int Dd, const float *y_in, int Dy,
                            int B, int H, int W, int Cp, float *packed, float *canvas_plane, void *stream);
/* canvas channel update used by box_model (box_model.py:500-504):
 * canvas = max(canvas, ysel - ysel*noise). ysel,noise [B,H,W]. */
int ra_canvas_max_f32(float *img, int Ci, int canvas_chan, const float *ysel, const float *noise,
                      int B, int H, int W, void *stream);

/* Stand-alone eval BatchNorm / affine (nnlib.batch_norm with phase_train=False,
 * nnlib.py:113-119): y[p,c] = relu?(x[p,c]*scale[c] + shift[c]), p < npix. */
int ra_affine_act_f32(const float *x, const float *scale, const float *shift, size_t npix, int C,
                      int relu, float *y, void *stream);
/* Stand-alone nnlib.max_pool (nnlib.py:15-25): ksize = stride = ratio, 'SAME' (-inf pad).
 * x [B,H,W,C] -> y [B,ceil(H/ratio),ceil(W/ratio),C]. */
int ra_max_pool_f32(const float *x, int B, int H, int W, int C, int ratio, float *y, void *stream);

/* ------------------------------------------------------------------------------------
 * Loss / statistics head of the training graph, forward only (full_model.py:913-1097).
 *
 * ra_pair_stats_f32 — modellib.f_iou(a, b, pairwise=True) (modellib.py:124-155),
 *   f_iou(a > 0.5, b, pairwise=True) (full_model.py:1064-1065) and f_dice(a > 0.5, b,
 *   pairwise=True) (modellib.py:71-104) in ONE pass over a [B,N,H*W] and b [B,M,H*W]
 *   (N, M <= 32, H*W % 4 == 0, 16-byte aligned).  Outputs (each nullable): iou_soft,
 *   iou_hard, dice_hard [B,N,M]; sum_a [B,N], sum_b [B,M] = per-instance pixel sums; inter
 *   [B,N,M] = the raw intersections sum(a*b) (exact integers for binary masks up to 2^24
 *   pixels); sum_a_hard [B,N] = pixel counts of (a > 0.5).
 *   ws: device scratch of ra_pair_stats_workspace_floats(B, H*W) floats.
 * ra_gt_box_f32 — modellib.get_gt_box (modellib.py:663-701) with center_shift_ratio 0:
 *   params [B,T,8] = top_left (y,x), bot_right (y,x) as returned by the reference, then the
 *   padded rectangle (tl_y, tl_x, br_y, br_x) the mask is filled with; box (nullable)
 *   [B,T,H,W] = the filled rectangle mask.  ws: ra_gt_box_workspace_floats(B, T) device floats.
 * ra_segm_match_f32 — modellib.f_segm_match (modellib.py:382-415): mask with s_gt, quantise
 *   to 1e-6, + 1e-5, Hungarian (device), mask again.  status: int[B] as ra_hungarian_f32_dev.
 * ra_loss_stats_f32 — every scalar of full_model.py:941-1081 for box_loss_fn = 'iou' and
 *   segm_loss_fn 0 = 'iou' / 1 = 'wt_cov': out[RA_STAT_COUNT] indexed by RA_STAT_*.
 *   sum_gt [B,T] = per-instance sums of y_gt (f_coverage_weight, modellib.py:277-289);
 *   ws: ra_loss_stats_workspace_floats(B) device floats.
 * ---------------------------------------------------------------------------------- */
enum {
  RA_STAT_LOSS = 0, RA_STAT_BOX_LOSS, RA_STAT_SEGM_LOSS, RA_STAT_CONF_LOSS, RA_STAT_IOU_SOFT,
  RA_STAT_IOU_SOFT_BOX, RA_STAT_WT_COV_SOFT, RA_STAT_UNWT_COV_SOFT, RA_STAT_IOU_HARD,
  RA_STAT_WT_COV_HARD, RA_STAT_UNWT_COV_HARD, RA_STAT_DICE, RA_STAT_COUNT_ACC, RA_STAT_DIC,
  RA_STAT_DIC_ABS, RA_STAT_COUNT
};
size_t ra_pair_stats_workspace_floats(int B, int HW);
int ra_pair_stats_f32(const float *a, const float *b, int B, int N, int M, int HW, float *ws,
                      size_t ws_floats, float *iou_soft, float *iou_hard, float *dice_hard,
                      float *sum_a, float *sum_b, float *inter, float *sum_a_hard, void *stream);
/* ra_pair_stats_f32 with a's planes addressed through strides (in floats, multiples of 4): a[img][row] starts at
 * img * a_img + row * a_row.  The training step keeps the masks of its T timesteps timestep-major ([T,B,H,W]: a_img = H*W,
 * a_row = B*H*W) — the pairwise IoU reads them in place instead of through a transposed copy. */
int ra_pair_stats_strided_f32(const float *a, size_t a_img, size_t a_row, const float *b, int B, int N, int M, int HW, float *ws,
                              size_t ws_floats, float *iou_soft, float *iou_hard, float *dice_hard, float *sum_a, float *sum_b,
                              float *inter, float *sum_a_hard, void *stream);
/* Soft IoU (modellib.f_iou, modellib.py:124-155) of one map per image, box [B,H,W], against the T rectangles
 * ra_gt_box_f32 fills (params [B,T,8], fields 4..7): iou [B,T] — the row the training graph takes per timestep
 * (full_model.py:744-758) without reading the T rectangle planes. */
size_t ra_box_iou_rects_workspace_floats(int B);
int ra_box_iou_rects_f32(const float *box, const float *params, int B, int T, int H, int W, float *ws,
                         size_t ws_floats, float *iou, void *stream);
size_t ra_gt_box_workspace_floats(int B, int T);
int ra_gt_box_f32(const float *y_gt, int B, int T, int H, int W, float padding_ratio,
                  float min_padding, float *ws, size_t ws_floats, float *params, float *box,
                  void *stream);

/*
 * ra_knob_setup_f32 — the training step's noisy ground-truth attention and knob masks from the partials ra_gt_box_f32
 * left in ITS workspace (same B, T; the call must come after it on the stream): modellib.get_gt_attn with per-instance
 * padding ratio pad [B,T] and centre shift [B,T,2] (full_model.py:567-577; modellib.py:688-701) -> ctr, size [B,T,2]
 * (an empty instance: top-left 0, bottom-right 2 * min_padding), and knob_box / knob_segm [B,T] = (u <= min(sched[k] *
 * scale_t, 1)), scale_t = 1 + log(1 + 3 t) with timescale (full_model.py:596-625); sched = 2 device floats (the
 * probabilities of this step).  One launch on B T numbers; float32 operations in the element-wise form's order.
 */
int ra_knob_setup_f32(const float *gt_box_ws, int B, int T, const float *pad, const float *shift, const float *u_box,
                      const float *u_segm, const float *sched, float min_padding, int timescale, float *ctr, float *size,
                      float *knob_box, float *knob_segm, void *stream);
size_t ra_segm_match_workspace_bytes(int B, int N);
int ra_segm_match_f32(const float *iou, const float *s_gt, int B, int N, void *ws, size_t ws_bytes,
                      float *match, int *status, void *stream);
/* ... with the B problems solved on HOST cores (ra_hungarian_f32 on up to `threads` threads) as a host function of the stream — a host
 * node of the graph when the stream is capturing (round 6): precondition kernel -> D2H copy into `pinned` -> host solve -> H2D ->
 * re-mask.  The device solver's launch lasts as long as its slowest problem (1.7 ms for a cfg4 step's 16 x 16 problems, on the
 * step's critical path); a host core needs ~0.5 ms per problem and the problems run side by side.  w_dev: B N N floats of device
 * scratch; pinned: page-locked host memory of ra_segm_match_host_block_bytes() (16-byte aligned) that carries the host function's
 * arguments and staging — it must stay allocated, and unused by anyone else, as long as a graph that captured the call lives.
 * match / status: device outputs as ra_segm_match_f32's (status[b]: ra_hungarian_f32's return code for problem b). */
size_t ra_segm_match_host_block_bytes(int B, int N);
int ra_segm_match_host_f32(const float *iou, const float *s_gt, int B, int N, float *w_dev, void *pinned, size_t pinned_bytes,
                           int threads, float *match, int *status, void *stream);
int ra_loss_stats_f32(const float *iou_soft, const float *iou_hard, const float *dice,
                      const float *match_real, const float *iou_box, const float *match_box,
                      const float *s_out, const float *s_gt, const float *sum_gt, int B, int T,
                      int fixed_order, int segm_loss_fn, float loss_mix_ratio, float *ws,
                      size_t ws_floats, float *out, void *stream);
size_t ra_loss_stats_workspace_floats(int B);

/* ------------------------------------------------------------------------------------
 * Evaluation post-processing and metrics (utils/postprocess.py, analysis.py:314-760).
 *
 * ra_postprocess_f32 — apply_confidence (postprocess.py:15-29), apply_one_label (:32-52),
 *   apply_threshold (:5-12) and, with fg [B,H,W] != NULL, mask_foreground (:139-147) in one
 *   pass: y_bin[b,t,p] = (t == argmax_t' y*s) && (max_t' y*s > thresh) [* fg]; s_hard
 *   (nullable) [B,T] = s_out > 0.5; union_out (nullable) [B,H,W] = max_t y_bin.
 * ra_union_f32 — y.max(axis=0) per image (analysis.py:547,570).
 * ra_remove_tiny_f32 — remove_tiny (postprocess.py:109-136): instance planes whose size
 *   (sizes [B,T], e.g. sum_a of ra_pair_stats_f32) is <= threshold are zeroed, conf too.
 * ra_eval_metrics_f32 — from inter [B,T,T] / sum_a / sum_b of the BINARY masks (outputs = a,
 *   ground truth = b) and s_gt: iou_pairwise (nullable) [B,T,T] (analysis.py:314-334); stats
 *   [B,RA_EVAL_COUNT]; inst (nullable) [B,RA_EVALI_COUNT,T].  fg_inter/fg_a/fg_b [B]
 *   (nullable together) = |union_a & union_b|, |union_a|, |union_b|; a_in_fgb [B,T] =
 *   |a_i & union_b|, b_in_fga [B,T] = |b_j & union_a| (both nullable).
 * ---------------------------------------------------------------------------------- */
enum {
  RA_EVAL_SBD = 0, RA_EVAL_WT_COV, RA_EVAL_UNWT_COV, RA_EVAL_FG_IOU, RA_EVAL_FG_DICE, RA_EVAL_FP,
  RA_EVAL_FN, RA_EVAL_COUNT_ACC, RA_EVAL_COUNT_MSE, RA_EVAL_DIC, RA_EVAL_DIC_ABS, RA_EVAL_NUM_OBJ,
  RA_EVAL_COUNT_OUT, RA_EVAL_COUNT
};
enum {
  RA_EVALI_OBJ_PR = 0, RA_EVALI_OBJ_RE, RA_EVALI_PIX_PR, RA_EVALI_PIX_RE, RA_EVALI_HAS_OUT,
  RA_EVALI_IS_GT, RA_EVALI_COUNT
};
int ra_postprocess_f32(const float *y_out, const float *s_out, int B, int T, int H, int W,
                       float thresh, const float *fg, float *y_bin, float *s_hard,
                       float *union_out, void *stream);
int ra_union_f32(const float *y, int B, int T, int HW, float *union_out, void *stream);
/* The evaluator's cv2 steps as plain kernels on N = B*T planes (full_model_eval.py:112-118):
 * ra_dilate_f32 — morph_single (postprocess.py:63-72): cv2.dilate(plane, ones(2 radius + 1)^2), out-of-image pixels ignored.
 * ra_resize_linear_f32 + ra_bilateral5_f32 — upsample_single (postprocess.py:93-106): cv2.resize(..., INTER_LINEAR) (pixel
 *   centres aligned, float32 two-tap weights) and cv2.bilateralFilter(b, 5, sigma_color, sigma_space) (circular radius-2
 *   neighbourhood, BORDER_REFLECT_101, the exact exponential where cv2 interpolates a table).  out != y. */
int ra_dilate_f32(const float *y, int N, int H, int W, int radius, float *out, void *stream);
int ra_resize_linear_f32(const float *y, int N, int Hs, int Ws, int H, int W, float *out, void *stream);
int ra_bilateral5_f32(const float *y, int N, int H, int W, float sigma_color, float sigma_space, float *out, void *stream);
int ra_remove_tiny_f32(float *y_bin, const float *sizes, float *conf, int B, int T, int HW,
                       float threshold, void *stream);
int ra_eval_metrics_f32(const float *inter, const float *sum_a, const float *sum_b,
                        const float *s_gt, const float *fg_inter, const float *fg_a,
                        const float *fg_b, const float *a_in_fgb, const float *b_in_fga, int B,
                        int T, float *iou_pairwise, float *stats, float *inst, void *stream);

/* In-graph augmentation, image_ops.random_transformation (image_ops.py:9-113) for given random
 * draws: zero-pad by `padding`, crop H x W at (off_y, off_x) in [0, 2*padding] (one offset per
 * batch), reverse along H (flip_v) / W (flip_h), then transpose H <-> W (needs H == W).
 * x, out: [N,H,W,C]; instance masks [B,T,H,W] go in as N = B*T, C = 1.  out != x.
 * The colour jitter (:99-103) is ra_colour_jitter_f32 below. */
int ra_random_transform_f32(const float *x, int N, int H, int W, int C, int padding, int off_y,
                            int off_x, int flip_v, int flip_h, int transpose, float *out,
                            void *stream);
/* The colour jitter of the same augmentation (image_ops.py:99-103,116-180: random_hue(0.1), random_saturation(0.9, 1.1),
 * tf.image.random_brightness(0.1), tf.image.random_contrast(0.9, 1.1)) for given draws, one of each per batch: RGB -> HSV,
 * hue = (hue + hue_delta + 1) mod 1, saturation = clip(saturation * factor, 0, 1), HSV -> RGB, + brightness_delta (no
 * clipping: float images), then (x - mean) * contrast_factor + mean with the mean of each image and channel.  TensorFlow's
 * kernels restated from their published algorithm; they cannot be run here.  x, out: [B,HW,3] (out may
 * be x); ws: ra_colour_jitter_workspace_floats(B) floats. */
size_t ra_colour_jitter_workspace_floats(int B);
int ra_colour_jitter_f32(const float *x, int B, int HW, float hue_delta, float saturation_factor, float brightness_delta,
                         float contrast_factor, float *ws, size_t ws_floats, float *out, void *stream);

/* out[b,p] = sum_t w[b,t] * y[b,t,p]: the ground-truth instance box_model's greedy match picks
 * (box_model.py:487-499).  Terms with w == 0 are skipped (0 * x is not evaluated). */
int ra_weighted_sum_f32(const float *w, const float *y, int B, int T, int HW, float *out,
                        void *stream);

/* ------------------------------------------------------------------------------------
 * The Cityscapes output stage behind the decode loop (csrc/ra_instance_class.hip): the foreground mask of the
 * pre-stage's semantic map and a semantic class for every decoded instance.  sem is the semantic map at network size,
 * [B,Hs,Ws,C] channel-last (channel 0 = background); H x W is the labels' size.  "Resized" below is
 * cv2.resize(plane, (W, H)) with its default INTER_LINEAR in float32 (the arithmetic of ra_resize_linear_f32 with the
 * source coordinate (d + 0.5) * (src / dst) - 0.5 evaluated in double as cv2 does); no full-size map is ever written.
 *
 * ra_sem_foreground_f32 — cityscapes_eval.py:166-176: fg[b,r,c] = C == 1 ? resized(sem) > thresh
 *   : resized(sem[..., 0]) <= 1 - thresh  (FG_THRESHOLD = 0.3 there); fg [B,H,W] of 0 / 1.  1 <= C <= 16.
 * ra_instance_class_vote_f32 — analysis.py:235-237: vote[b,t,c] = mean over the H * W pixels of
 *   y[b,t,r,c'] * resized(sem[b,...,c])[r,c'] for any float y [B,T,H,W] (soft values, several instances on a pixel).  y is
 *   read once, with 16-byte loads when H * W % 4 == 0 and y is 16-byte aligned (element loads otherwise).  Every workgroup
 *   leaves its partial sums in ws (ra_instance_class_vote_workspace_floats(B, T, H, W, C) floats) and a second launch adds
 *   them in a fixed order: no float atomics, the same bits on every run.  With conf [B,T] != NULL that launch also does
 *   ra_instance_class_pick_f32's work (class_idx / label_id nullable).  1 <= T <= 32, 2 <= C <= 16, else RA_E_SHAPE and
 *   nothing is launched.
 * ra_instance_class_pick_f32 — analysis.py:232,251-261: an instance is written when conf > 0.5 and vote[0] <= 0.7, with
 *   class_idx = argmax(vote[1:]) (first maximum) and label_id = (24, 25, 26, 27, 28, 31, 32, 33)[class_idx] (person,
 *   rider, car, truck, bus, train, motorcycle, bicycle, analysis.py:203-210; -1 beyond the table); otherwise both are -1.
 *   vote[0] is a mean over the whole image, so the gate almost never closes: the reference's rule, kept.
 * ---------------------------------------------------------------------------------- */
int ra_sem_foreground_f32(const float *sem, int B, int Hs, int Ws, int C, int H, int W, float thresh, float *fg,
                          void *stream);
size_t ra_instance_class_vote_workspace_floats(int B, int T, int H, int W, int C);
int ra_instance_class_vote_f32(const float *y, const float *sem, int B, int T, int H, int W, int Hs, int Ws, int C,
                               const float *conf, float *ws, size_t ws_floats, float *vote, int *class_idx,
                               int *label_id, void *stream);
int ra_instance_class_pick_f32(const float *vote, const float *conf, int B, int T, int C, int *class_idx, int *label_id,
                               void *stream);

/* ------------------------------------------------------------------------------------
 * The same stage behind an EXTERNAL semantic segmentation given as a label image (csrc/ra_label_vote.hip): the
 * reference's --lrr_seg path, cityscapes_eval.py:162-164 and 212-232, where the label image becomes a one-hot [H,W,9] map,
 * the foreground mask is "one of the eight thing classes" and the vote of analysis.py:235-237 counts pixels per class.
 * y float32 [B,T,H,W] are the masks after upsample and apply_confidence (cityscapes_eval.py:179-180), labels uint8 [B,H,W]
 * the label image at the same size, lut 256 bytes ON THE HOST (copied into the launch): label value -> 0 (background or
 * ignored) or 1 .. 8 = person .. bicycle in the order of analysis.py:203-210.  Per pixel p: t* = the first maximum of
 * y[b,:,p] (postprocess.py:45), v = y[b,t*,p], c = lut[labels[b,p]].  y is read with 16-byte loads when H * W % 4 == 0 and
 * it is 16-byte aligned, labels with 4-byte loads when H * W % 4 == 0 and they are 4-byte aligned, element loads otherwise.
 * 1 <= T <= 32, B <= 65535, H * W <= 2^30, every lut entry <= 8 — and 1 <= K <= 16 for the sweep — else RA_E_SHAPE and
 * nothing is launched.
 *
 * ra_label_vote_sweep_f32 — the threshold loop of cityscapes_eval.py:183-189 with the vote and the pick of
 *   analysis.py:232-261, for all K thresholds (a HOST array) from ONE read of y.  counts int32 [K,B,T,8], zeroed by the call:
 *   counts[k,b,t*,c-1] = the pixels with c > 0 and v > (float)thresholds[k] — strict and in float32, postprocess.py:12 on a
 *   float32 array.  The thresholds may be unsorted and repeat.  Integer counters (LDS, then global atomics): exact at any
 *   size, the same bits on every run.  Then, walking the thresholds in list order (all outputs with a leading K axis):
 *     sizes int32 [K,B,T]     the sum of counts over the classes: the plane's pixels after mask_foreground
 *     keep uint8 [K,B,T]      remove_tiny == 0 (postprocess.py:115) or sizes > remove_tiny (:131)
 *     conf float [K,B,T]      conf[k] = keep[k] ? conf[k-1] : 0, conf[-1] = conf_in [B,T]: carried from threshold to
 *                             threshold as cityscapes_eval.py:188-189 re-assigns it
 *     vote float [K,B,T,9]    vote[..., 0] = 0 (no background pixel is left under a mask), vote[..., 1+c] = counts /
 *                             (H * W) rounded once; all zero for a plane that is not kept
 *     class_idx, label_id int32 [K,B,T]   conf[k] > 0.5: the first maximum of the counts and its label of
 *                             (24, 25, 26, 27, 28, 31, 32, 33); otherwise -1.  The gate vote[0] <= 0.7 of analysis.py:252 is
 *                             always open here.
 *   The integer counts define the class; the reference's float32 means of means equal counts / (H * W) exactly when H and
 *   W are powers of two and can otherwise differ in near-ties of two classes.
 * ra_label_planes_f32 — one threshold's planes, one read and one write: y_bin[b,t,p] = (t == t*) && v > (float)thresh &&
 *   c > 0 && keep[b,t] as 0 / 1 floats; keep uint8 [B,T], NULL = keep all.  For thresh >= 0 this is apply_one_label ->
 *   apply_threshold -> mask_foreground -> remove_tiny (postprocess.py:5-52, 109-145) to the bit.  (Below zero the
 *   reference's chain also marks every plane that lost the arg-max, whose one-label value 0 exceeds the threshold; here
 *   only the arg-max plane is ever marked, in the planes and in the counts.)
 * ---------------------------------------------------------------------------------- */
int ra_label_vote_sweep_f32(const float *y, const unsigned char *labels, const unsigned char *lut, int B, int T, int H,
                            int W, const double *thresholds, int K, const float *conf_in, int remove_tiny, int *counts,
                            int *sizes, unsigned char *keep, float *conf, float *vote, int *class_idx, int *label_id,
                            void *stream);
int ra_label_planes_f32(const float *y, const unsigned char *labels, const unsigned char *lut, int B, int T, int H, int W,
                        double thresh, const unsigned char *keep, float *y_bin, void *stream);

/* ------------------------------------------------------------------------------------
 * The matching step of the Cityscapes instance-level evaluation (csrc/ra_instance_overlap.hip), cited as lines of
 * data_api/cityscapes_scripts/evaluation/evalInstanceLevelSemanticLabeling.py unless a file is named.  gt_ids is int32
 * [B,H,W]: the values of *_gtFine_instanceIds.png, a label id below 1000 or labelId * 1000 + k.  H * W < 2^31.
 *
 * ra_gt_instance_catalog_i32 — instances2dict.py:37-40 with instance.py:26-27, np.unique(gt, return_counts=True) per
 *   image: ids[b, 0 .. count[b]) the distinct ids in ascending order (-1 beyond), pixels[b, .] their pixel counts (0
 *   beyond); ids, pixels int32 [B, RA_OVERLAP_MAX_GT], count, status int32 [B].  Ids live in [0, 65535], the range of the
 *   16-bit PNG, and an image has at most RA_OVERLAP_MAX_GT distinct ids: that cap is a constant of the kernels and rests on
 *   no measurement of the real dataset (which this project cannot read).  status[b] is 0 or a sum of RA_GT_STATUS_RANGE
 *   (an id outside [0, 65535] was met) and RA_GT_STATUS_COUNT (more distinct ids than the cap: the smallest
 *   RA_OVERLAP_MAX_GT of those kept are listed); such ids are counted in a reject slot and never index anything, and the
 *   other images of the batch are unaffected.  ws: ra_gt_instance_catalog_workspace_ints(B, H, W) ints.
 * ra_instance_overlap_f32 — :306-307, :333: a pixel belongs to prediction t of image b where y[b,t] != 0 (y float32
 *   [B,T,H,W]); pred_pixels[b,t] is their number and inter[b,t,g] the number of them on catalogue entry g (gt_ids ==
 *   ids[b,g]; 0 for g >= count[b]); inter int32 [B,T,RA_OVERLAP_MAX_GT], pred_pixels int32 [B,T].  ids, count: what
 *   ra_gt_instance_catalog_i32 wrote.  Pixels whose id is not in the catalogue count in pred_pixels only.  y and gt_ids
 *   are read once each (16-byte loads when H * W % 4 == 0 and both are 16-byte aligned); integer counters, workgroup
 *   partials in ws (ra_instance_overlap_workspace_ints(B, T, H, W) ints) added by a second launch: exact, and the same on
 *   every run.  1 <= T <= 32, else RA_E_SHAPE and nothing is launched.
 * ---------------------------------------------------------------------------------- */
#define RA_OVERLAP_MAX_GT 256
#define RA_GT_STATUS_RANGE 1
#define RA_GT_STATUS_COUNT 2
size_t ra_gt_instance_catalog_workspace_ints(int B, int H, int W);
int ra_gt_instance_catalog_i32(const int *gt_ids, int B, int H, int W, int *ws, size_t ws_ints, int *ids, int *pixels,
                               int *count, int *status, void *stream);
size_t ra_instance_overlap_workspace_ints(int B, int T, int H, int W);
int ra_instance_overlap_f32(const float *y, const int *gt_ids, const int *ids, const int *count, int B, int T, int H, int W,
                            int *ws, size_t ws_ints, int *inter, int *pred_pixels, void *stream);

/* ------------------------------------------------------------------------------------
 * The Cityscapes pixel-level evaluation (csrc/ra_pixel_eval.hip), cited as lines of
 * data_api/cityscapes_scripts/evaluation/evalPixelLevelSemanticLabeling.py.  Label ids run from 0 to 33
 * (RA_PIXEL_LABELS = 34, helpers/labels.py); the thing labels are (24, 25, 26, 27, 28, 31, 32, 33) as above, the instance
 * categories human = {24, 25} and vehicle = {26 .. 33}, caravan and trailer included, as generateInstanceStats builds them
 * (:182-200).  gt_ids int32 [B,H,W] are *_gtFine_instanceIds.png values, ids / count their catalogue as
 * ra_gt_instance_catalog_i32 wrote it.  H * W < 2^31.
 *
 * ra_sem_labels_u8 — the label image of the pre-stage's semantic map: sem float32 [B,Hs,Ws,C] (channel 0 the background,
 *   2 <= C <= 9) -> labels uint8 [B,H,W].  Every channel is resized to H x W with the linear resample of
 *   ra_sem_foreground_f32 / ra_instance_class_vote_f32 (cv2.resize INTER_LINEAR, float32, the source coordinate in double);
 *   the FIRST maximum over the channels wins; channel 0 gives label 0, channel c >= 1 the thing label (24, ..)[c - 1].  All
 *   channels of a pixel go through the same sequence of operations, so channels equal at the four taps stay exactly equal.
 * ra_pixel_confusion_u8 / ra_pixel_confusion_sem_f32 — evaluatePair (:532-615) for B images: the prediction is a label
 *   image pred uint8 [B,H,W], or (_sem_f32) the label ra_sem_labels_u8 would give for sem, evaluated on the fly by the same
 *   device function with no full-size plane written.  gt_labels uint8 [B,H,W] are the *_gtFine_labelIds.png values; NULL:
 *   the label of a pixel is id < 1000 ? id : id / 1000, as the instance images encode it.
 *     conf unsigned 64-bit [34,34]   conf[g][p] += the pixels with ground-truth label g and predicted label p (:566-573).
 *                                    ADDED to what is there: a data set is many calls.
 *     inst_tp int32 [B,RA_OVERLAP_MAX_GT]      per catalogue slot k: the pixels with gt_ids == ids[k] whose prediction
 *                                    equals ids[k] / 1000 (:588-591)
 *     inst_cat_tp int32 [B,RA_OVERLAP_MAX_GT]  those whose prediction lies in the instance category of ids[k] / 1000
 *                                    (:579, :603-606); 0 where that label is in neither category.  Both are written for every
 *                                    slot, ids <= 1000 included (the host skips them, :581), and are 0 beyond count[b].
 *     status int32 [B]               0, or a sum of RA_PIXEL_STATUS_GT (a ground-truth label above 33 was met, :570-571) and
 *                                    RA_PIXEL_STATUS_PRED (a predicted label above 33).  A pixel with such a label is
 *                                    counted in no cell of conf, and nothing is indexed by an unchecked value; every other
 *                                    pixel, of this image and of the others, is counted as usual.
 *   A workgroup walks tiles of RA_PIXEL_TILE pixels of one image (16-byte loads of gt_ids and 4-byte loads of the label
 *   images when H * W % 4 == 0 and the pointers are aligned so, element loads otherwise) with its counters in LDS and
 *   leaves them in ws (ra_pixel_confusion_workspace_ints(B, H, W) ints); a finishing launch adds them, per image in int32
 *   and over the images in 64 bits.  No global atomics: exact, the same on every run.  B <= 65535, 2 <= C <= 9, else
 *   RA_E_SHAPE and nothing is launched.
 * ---------------------------------------------------------------------------------- */
#define RA_PIXEL_LABELS 34
#define RA_PIXEL_TILE 1024
#define RA_PIXEL_STATUS_GT 1
#define RA_PIXEL_STATUS_PRED 2
int ra_sem_labels_u8(const float *sem, int B, int Hs, int Ws, int C, int H, int W, unsigned char *labels, void *stream);
size_t ra_pixel_confusion_workspace_ints(int B, int H, int W);
int ra_pixel_confusion_u8(const unsigned char *pred, const int *gt_ids, const unsigned char *gt_labels, const int *ids,
                          const int *count, int B, int H, int W, int *ws, size_t ws_ints, unsigned long long *conf,
                          int *inst_tp, int *inst_cat_tp, int *status, void *stream);
int ra_pixel_confusion_sem_f32(const float *sem, int Hs, int Ws, int C, const int *gt_ids, const unsigned char *gt_labels,
                               const int *ids, const int *count, int B, int H, int W, int *ws, size_t ws_ints,
                               unsigned long long *conf, int *inst_tp, int *inst_cat_tp, int *status, void *stream);

/* ------------------------------------------------------------------------------------
 * The label stage in front of training and of the pre-stage's evaluation (csrc/ra_labels.hip): the ground truth the
 * reference's setup_cityscapes.py / setup_kitti.py / setup_cvppp.py assemble (data_api/ins_seg_assembler.py:85-155,
 * sep_labels.py, orientation.py:31-85) as ins_seg_dataset.py:158-172,216-236,257-271 reads it back, from instance-id images.
 *
 * ra_labels_assemble_i32 — gt_ids int32 [B,Hf,Wf] and ids, count as ra_gt_instance_catalog_i32 wrote them for it: the
 *   catalogue of the FULL image (sep_labels takes np.unique of it), so an instance that vanishes at network size still
 *   counts as an object.  dataset: RA_LABELS_PLAIN (cvppp.py:49-63, kitti.py:51-65) — every id != 0 is an instance, one
 *   semantic class; RA_LABELS_CITYSCAPES (cityscapes.py:88-119) — an id is an instance iff id > 1000 and id / 1000 is one of
 *   the labels (24, 25, 26, 27, 28, 31, 32, 33) of ra_instance_class_pick_f32, its class that label's position 0 .. 7; every
 *   other id (stuff, ids up to 1000, caravan / trailer) is background.  Network pixel (r, c) reads full-size pixel
 *   (min(floor(r * sy), Hf - 1), min(floor(c * sx), Wf - 1)), sy = 1.0 / ((double)H / Hf) in double and sx likewise: the
 *   form of cv2.resize(..., INTER_NEAREST) (ins_seg_assembler.py:125,145), restated from OpenCV's source.  Outputs, each
 *   nullable and then skipped:
 *     num_obj int32 [B]            accepted catalogue entries
 *     s_gt float [B,T]             1 for t < min(num_obj, T) (:267-271), also for an instance that is empty at network size
 *     inst_id, area, sem_cls       int32 [B,T]: the id of slot t, its pixel count AT NETWORK SIZE, its class (0 under PLAIN);
 *                                  -1 / 0 / -1 beyond num_obj
 *     y_gt float [B,T,H,W]         slot t = the 0 / 1 mask of inst_id[b,t], zero beyond num_obj.  Slots are in descending
 *                                  order of area (:169-172, np.argsort(area)[::-1]); equal areas: the larger catalogue
 *                                  index (the larger id) first — a stable ascending sort read backwards, which is what
 *                                  NumPy gives up to 16 elements; beyond that NumPy's order is not stable, so this is the
 *                                  library's rule
 *     d_cls uint8 [B,H,W]          orientation.get_orientation(all instances at network size, encoding='class'): over ALL
 *                                  accepted instances, not the first T (ins_seg_assembler.py:136-139); 0 on the background.
 *                                  Per pixel in double, in the reference's order: v = (r - cy, c - cx), centroid = sum /
 *                                  (area + 1e-7); o = (v + 1e-8) / (sqrt(v . v) + 1e-7); a = asin(o_y) folded by the signs of
 *                                  o_x, o_y; a += pi / 8; class = floor((a + pi) * 8 / 2 / pi) mod 8.  The centroid pixel
 *                                  gets o = (0.1, 0.1), class 0 is shared with the background: the reference's quirks, kept
 *     d_gt float [B,H,W,8]         d_gt[..., o] = (d_cls == o) (:257-262): channel 0 is 1 on the background
 *     c_gt float [B,H,W,nc]        PLAIN: nc = 1, the union of the instances; CITYSCAPES: nc = 9, channel 1 + k the union of
 *                                  class k's instances, channel 0 = 1 - max of the others (:216-236)
 *     fg_gt_full uint8 [B,Hf,Wf]   1 where the dataset rule accepts the id (fg_model_eval.py:142-143)
 *   Launches on one stream: the moments of the sampled positions (integer counters in LDS, workgroup partials in ws), one
 *   workgroup per image that adds them in a fixed order, applies the rule and ranks, one fill that writes all T planes of its
 *   pixels (16-byte stores when H * W % 4 == 0 and the outputs are 16-byte aligned), and the full-size foreground.  No
 *   floating-point atomics, nothing indexed by an id, the same bits on every run.  An image whose catalogue status is not
 *   0 keeps that status word for the caller to report; its outputs describe the listed ids only, the other images are
 *   unaffected.  1 <= T <= RA_LABELS_MAX_T, 1 <= H <= Hf, 1 <= W <= Wf, Hf * Wf < 2^31, else RA_E_SHAPE before anything is
 *   read or launched.  ws: ra_labels_workspace_bytes(B, H, W) bytes, 8-byte aligned.
 * ---------------------------------------------------------------------------------- */
#define RA_LABELS_PLAIN 0
#define RA_LABELS_CITYSCAPES 1
#define RA_LABELS_MAX_T 32
size_t ra_labels_workspace_bytes(int B, int H, int W);
int ra_labels_assemble_i32(const int *gt_ids, const int *ids, const int *count, int B, int Hf, int Wf, int H, int W, int T,
                           int dataset, void *ws, size_t ws_bytes, int *num_obj, float *s_gt, int *inst_id, int *area,
                           int *sem_cls, float *y_gt, unsigned char *d_cls, float *d_gt, float *c_gt,
                           unsigned char *fg_gt_full, void *stream);

/* ------------------------------------------------------------------------------------
 * The image stage in front of the label stage (csrc/ra_image.hip): the network's input x from the full-size colour image,
 * data_api/ins_seg_assembler.py:116 (cv2.resize(img, inp_shape, interpolation=cv2.INTER_CUBIC) on the uint8 BGR array of
 * cv2.imread) as ins_seg_dataset.py:149 reads it back (x / 255 in float32), and the row filters of the PNG files the images
 * come in.  cv2 is not part of this stack and was never run: what follows RESTATES the fixed-point recipe its source has for
 * 8-bit images, and equality is claimed with this statement.
 *
 * One axis of source length S and destination length D: scale = (double)S / D; f = (float)((d + 0.5) * scale - 0.5);
 *   s = floor(f), t = f - s in float32; with A = -0.75 the float32 weights
 *     c0 = ((A*(t+1) - 5A)*(t+1) + 8A)*(t+1) - 4A      c1 = ((A+2)*t - (A+3))*t*t + 1
 *     c2 = ((A+2)*(1-t) - (A+3))*(1-t)*(1-t) + 1       c3 = 1 - c0 - c1 - c2
 *   q[k] = (short)rint(c[k] * 2048), half to even, the sum NOT corrected (2047 and 2049 occur); tap k reads source index
 *   clamp(s - 1 + k, 0, S - 1).  A pixel: h = sum_k qx[k] * src[..] in int32 along x, v = sum_k qy[k] * h_k along y,
 *   out = clamp((v + (1 << 21)) >> 22, 0, 255), an arithmetic shift.
 *
 * ra_resize_cubic_tables — HOST code, no GPU call: ofs[D] = s and coef[D][4] = q of one axis.  S, D >= 1, else RA_E_SHAPE.
 * ra_resize_cubic_u8 — src uint8 [N,Hs,Ws,C], C = 1 | 3, and the tables of the y axis (Hs -> H) and of the x axis (Ws -> W)
 *   in DEVICE memory -> dst_u8 uint8 [N,H,W,C] and / or dst_f32 float [N,H,W,C] = (float)level / 255.0f, a correctly
 *   rounded float32 division (NumPy's u8.astype(float32) / 255, bit for bit); a NULL output is skipped.  Any Hs, Ws, H, W
 *   >= 1, enlarging included; Hs * Ws * C < 2^31, the bytes of an output plane (H * W * C, x 4 with dst_f32) < 2^31,
 *   1 <= N <= 65535; anything else, a NULL src or a NULL table is RA_E_SHAPE before anything is launched.  One launch, no
 *   allocation, no synchronisation.  Source rows are staged with 16-byte loads when Ws * C % 16 == 0 and src is 16-byte
 *   aligned, the outputs are stored 4 values at a time when W * C % 4 == 0 and they are aligned (dst_u8 4, dst_f32 16
 *   bytes); the other forms read and write single bytes / floats.  Tap indices are clamped inside the kernel: tables of
 *   another shape give wrong pixels, never an access outside src.
 * ra_png_unfilter_u8 — HOST code, no GPU call: the filters of PNG specification 9.2 undone.  raw: H scanlines of one
 *   filter-type byte + stride bytes; bpp: bytes per complete pixel (1 .. 8, stride a multiple of it); out: uint8 [H,stride].
 *   A filter type above 4 or a bad size is RA_E_SHAPE and names the row.
 * ---------------------------------------------------------------------------------- */
int ra_resize_cubic_tables(int S, int D, int *ofs, short *coef);
int ra_resize_cubic_u8(const unsigned char *src, int N, int Hs, int Ws, int C, int H, int W, const int *ofs_y,
                       const short *coef_y, const int *ofs_x, const short *coef_x, unsigned char *dst_u8, float *dst_f32,
                       void *stream);
int ra_png_unfilter_u8(const unsigned char *raw, int H, int stride, int bpp, unsigned char *out);

/* ------------------------------------------------------------------------------------
 * The render stage behind the evaluators (csrc/ra_render.hip): the colour images the reference's analyzers write, composed
 * while the masks are on the device.  img is uint8 [B,H,W,3] in the memory order cv2.imwrite takes (B, G, R), the
 * convention of utils/png.read_colour8; colour tables are in that same order.  One launch each, no atomics, no workspace.
 *
 * ra_render_instances_u8 — y float32 [B,T,H,W], colour uint8 [B,T,3] (a table per image).  With u(v) = the float
 *   truncated to an integer, taken mod 256 (NumPy's .astype('uint8')), per pixel and channel k:
 *     RA_RENDER_ADD    analysis.py:137-147 (RenderInstanceAnalyzer): img_k = (sum_t u(y_t) * colour[b,t,k]) mod 256 — the
 *                      reference's uint8 product and its uint8 += both wrap; its `size > 0` gate changes nothing, an empty
 *                      plane adds zero.
 *     RA_RENDER_FIRST  analysis.py:166-187 (RenderGroundtruthInstanceAnalyzer): in the order t = 0 .. T - 1,
 *                      if img_k == 0: img_k = (u(y_t) * colour[b,t,k]) mod 256.  Decided PER CHANNEL, not per pixel
 *                      ((total_img == 0) is an [H,W,3] array there): a later overlapping plane fills exactly the channels the
 *                      earlier colour left at 0.
 *   The domain is finite 0 <= y <= 255 (binary masks in practice; a soft 0.7 gives 0); outside it the reference's cast is
 *   undefined and the bytes written here are unspecified.  y is read once: a lane takes four consecutive pixels with one
 *   16-byte load per plane and writes its 12 bytes as three dwords when H * W % 4 == 0, y is 16-byte and img 4-byte aligned;
 *   element loads and byte stores otherwise.  1 <= T <= RA_RENDER_MAX_T, planes up to 2^30 pixels, B <= 65535, else
 *   RA_E_SHAPE; another mode is RA_E_INVALID; nothing is launched then.
 * ra_render_orientation_u8 — fg_model_eval.py:128-132,154-164 with data_api/orientation.py:13-28: d float32 [B,Hs,Ws,C] at
 *   network size, mask float32 [B,H,W], wheel uint8 [C,3].  Every channel of d is resized to H x W with the linear
 *   resample of ra_sem_labels_u8 (cv2.resize INTER_LINEAR, float32, the source coordinate in double: the same device
 *   function), the FIRST maximum over the channels is the class, img = (uint8)(wheel[class] * mask).  No full-size plane of
 *   d is written.  The domain is mask = 0 or 1: beyond it the reference's float-to-uint8 cast of colour * mask is undefined.
 *   2 <= C <= 16, planes up to 2^30 pixels, B <= 65535, else RA_E_SHAPE and nothing is launched.
 * ---------------------------------------------------------------------------------- */
#define RA_RENDER_ADD 0
#define RA_RENDER_FIRST 1
#define RA_RENDER_MAX_T 1024
int ra_render_instances_u8(const float *y, int B, int T, int H, int W, const unsigned char *colour, int mode,
                           unsigned char *img, void *stream);
int ra_render_orientation_u8(const float *d, int B, int Hs, int Ws, int C, const float *mask, int H, int W,
                             const unsigned char *wheel, unsigned char *img, void *stream);

/* ------------------------------------------------------------------------------------
 * PNG output on the device (csrc/ra_png.hip): the deflate stage of utils/png.encode_gray8 / encode_colour8 for a batch of
 * images in device memory.  Per image a finished zlib stream leaves; the host wraps it (signature, IHDR, IDAT with
 * zlib.crc32 over the stream, IEND: utils/png.wrap).  The files decode to the pixels of the host writers' files; their
 * bytes differ, so the output stages use this only when asked (device_png).
 *
 * THE STREAM (three implementations agree on it byte for byte: the kernels, ra_png_deflate_host, tests/png_deflate_oracle.py)
 *   scanline  one filter-type byte 0, then the row: W bytes (grey, d = 1) or 3 W bytes in the FILE's order R, G, B (d = 3;
 *             the source is in cv2's memory order B, G, R and is swapped in the load).  Filter 0 on every row.
 *   segment   one scanline, n = 1 + W * bpp bytes, encoded on its own and ending on a byte boundary:
 *               a block with BFINAL = 0, BTYPE = 01 (the fixed Huffman code of RFC 1951 3.2.6), its tokens, end-of-block,
 *               then an empty stored block as a sync flush: bits 0, 00, zero bits up to the byte boundary, 00 00 FF FF.
 *   tokens    the greedy left-to-right run code at distance d: at byte i >= d of the segment, L = the number of following
 *             bytes, at most 258, that each equal the byte d before it; L >= 3: one match (length L, distance d), else the
 *             literal b[i].  The first d bytes are literals; no match reaches outside its segment.  Closed form, per maximal
 *             stretch of R positions with b[i] == b[i-d]: R / 258 matches of 258, then one match of R % 258 if that is >= 3,
 *             else R % 258 literals.
 *   stream    78 01, the segments of rows 0 .. H - 1, the final empty fixed block 03 00, the big-endian Adler-32 of all
 *             scanline bytes.
 *   bound     a literal takes at most 9 bits, a match of L >= 3 bytes at most 8 + 5 + 5 = 18 <= 9 L, so a segment takes at
 *             most 3 + 9n + 7 + 3 bits before padding: at most ceil(9n / 8) + 7 bytes with the pad and LEN/NLEN; a stream at
 *             most 8 + H * (ceil(9n / 8) + 7) bytes.
 *   Adler-32  per segment (A, B) from (1, 0), reduced per thread chunk (a colour row of 6145 bytes of 255 overflows 32-bit
 *             sums reduced only at the end); segments combine exactly: A = A1 + A2 - 1, B = B1 + B2 + n2 (A1 - 1) mod 65521.
 *   A run code within a row: masks and flat-colour images shrink to a few tens of KB (2.5 x what zlib level 6 makes of a
 *   flat-colour image, 6 - 7 x for a binary mask: profiles/png_device.txt), continuous-valued planes GROW; those stay with the host's zlib.
 *
 * Sources (kind): RA_PNG_GRAY8 uint8 [M,H,W]; RA_PNG_BGR8 uint8 [M,H,W,3] in B, G, R order; RA_PNG_F32 float [M,H,W],
 *   quantised in the load as (uint8)(v * 255.0f), what (y * 255).to(torch.uint8) gives for 0 <= v <= 1 (outside it the cast
 *   is undefined there and the bytes here unspecified).  plane (nullable): int32 [N], image i of the call is source image
 *   plane[i], indices may skip, repeat and reorder; NULL: image i is source image i and N <= M.  The host entry refuses an
 *   index outside [0, M) with RA_E_SHAPE; the device entry cannot read the list and clamps it in the kernel: wrong pixels,
 *   never an access outside src.
 *
 * ra_png_deflate_bound — bpp: 1 (grey and float sources) or 3.  *stream_bytes: the bound of one stream; *workspace_bytes: what
 *   ra_png_deflate_u8 needs for N such images (a 16-byte record and a worst-case slot per segment).
 * ra_png_deflate_u8 — every pointer, the plane list included, in DEVICE memory.  out: N streams back to back, stream i at
 *   out + offsets[i] with sizes[i] bytes (offsets[0] = 0, offsets[i + 1] = offsets[i] + sizes[i]); adler[i]: its Adler-32.
 *   Three plain launches on the stream (encode: a workgroup per scanline; scan: a workgroup per image; compact: a wave per
 *   segment), no allocation, no synchronisation, no workgroup waits for another.  Rows are staged with 16-byte loads when src
 *   is 16-byte aligned and W % 16 == 0 (float: W % 4 == 0), with element loads otherwise.
 * ra_png_deflate_host — HOST code, no GPU call: the same arguments in host memory (ws may be NULL), the rule above in plain
 *   sequential C++.  The same bytes as the device entry.
 * Refusals, all before anything is read, written or launched: a NULL src, out, sizes, offsets or adler, or another kind:
 *   RA_E_INVALID.  N < 1 or N > RA_PNG_MAX_IMAGES, M < 1, H < 1, W < 1, N > M without a plane list, scanlines above
 *   RA_PNG_MAX_ROW_BYTES (the segment and its bits wait in LDS), an image of 2^31 source bytes or a stream bound of 2^31, bpp
 *   other than 1 or 3 (bound query): RA_E_SHAPE.  out_bytes < N * stream bound, a NULL, short or not 16-byte aligned ws
 *   (device entry): RA_E_WORKSPACE.  The message names the argument.
 * ---------------------------------------------------------------------------------- */
#define RA_PNG_GRAY8 0
#define RA_PNG_BGR8 1
#define RA_PNG_F32 2
#define RA_PNG_MAX_ROW_BYTES 24576
#define RA_PNG_MAX_IMAGES 65535
int ra_png_deflate_bound(int N, int H, int W, int bpp, unsigned long long *stream_bytes, unsigned long long *workspace_bytes);
int ra_png_deflate_u8(const void *src, int kind, int M, int N, int H, int W, const int *plane, unsigned char *out,
                      size_t out_bytes, int *sizes, unsigned long long *offsets, unsigned int *adler, void *ws, size_t ws_bytes,
                      void *stream);
int ra_png_deflate_host(const void *src, int kind, int M, int N, int H, int W, const int *plane, unsigned char *out,
                        size_t out_bytes, int *sizes, unsigned long long *offsets, unsigned int *adler, void *ws,
                        size_t ws_bytes);

/* ------------------------------------------------------------------------------------
 * The second stream format of the device PNG encoder, "dynamic" (csrc/ra_png_dyn.hip): ONE dynamic-Huffman block per image with
 * the rows bit-contiguous, the literal / length code built on the device from the image's own histogram.  A 1024 x 2048 binary
 * mask takes about a fifth of the fixed format's bytes and 1.15 - 1.25 x what zlib level 6 makes of it (profiles/png_dynamic.txt).
 * The fixed format above keeps its bytes and stays the default.
 *
 * THE STREAM (three implementations agree on it byte for byte: the kernels, ra_png_deflate_dyn_host, tests/png_dynamic_oracle.py)
 *   scanline  as above: a filter-type byte 0, then W bytes (grey and float sources, d = 1) or 3 W bytes R, G, B (d = 3).
 *   tokens    as above: the greedy run code at distance d within a scanline; no match leaves its row.
 *   framing   78 01, then one block: BFINAL = 1, BTYPE = 10, the code header, the tokens of rows 0 .. H - 1 back to back at bit
 *             granularity (no per-row padding, no per-row block), one end-of-block symbol, zero bits up to the byte boundary,
 *             the big-endian Adler-32 of all scanline bytes.  No trailing empty block.
 *   lengths   THE RULE, a function of a histogram alone (ra_png_huffman_lengths): the used symbols (count > 0) sorted by
 *             (count, symbol index) are the leaves of a Huffman tree built with two queues — the sorted leaves and the internal
 *             nodes in the order they are made; each step takes the two smallest heads, a leaf before an internal node on a
 *             tie, and makes their sum a new internal node.  A symbol's length is its leaf's depth.  While the deepest leaf is
 *             deeper than the limit, every count c > 0 is replaced by (c + 1) >> 1 and the tree is built again (this ends: once
 *             every count is 1 the tree of at most 286 leaves is balanced at depth <= 9, of 19 leaves at depth <= 5).  Unused
 *             symbols get length 0; a histogram with one used symbol gives it length 1.  Codes are canonical (RFC 1951 3.2.2).
 *   literal / length code   over the 286 symbols from the image's histogram of its tokens, end-of-block counted once, limit 15.
 *             The filter byte and end-of-block are always in use, so the code is complete.  HLIT = (the last used symbol + 1) - 257.
 *   distance code   exactly one symbol in use, 0 for d = 1 and 2 for d = 3, always of length 1 (also in an image without a match):
 *             HDIST + 1 = 1 resp. 3 lengths, {1} resp. {0, 0, 1}; a match's distance is the single bit 0.  zlib accepts this
 *             incomplete one-code set.
 *   code-length code   the HLIT + 257 literal / length lengths and the HDIST + 1 distance lengths form one sequence.  A run of
 *             zeros is cut greedily: symbol 18 (11 .. 138 zeros) while at least 11 remain, then one symbol 17 (3 .. 10) if at
 *             least 3 remain, then single zeros; a run may cross from the literal / length into the distance lengths.  Every
 *             non-zero length is sent on its own; symbol 16 is not used.  The 19 code-length symbols are coded by THE RULE with
 *             limit 7 over the histogram of that symbol sequence; HCLEN + 4 = the last used position in the RFC's order (16, 17,
 *             18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15), at least 4.
 *   bound     the header: 16 (78 01) + 3 + 14 + 19 * 3 + at most 7 bits per entry of the sequence of at most 289 = 2113 bits.  A
 *             literal takes at most 15 bits, a match of L >= 3 bytes at most 15 + 5 + 1 = 21 <= 15 L, end-of-block at most 15:
 *             a stream of H scanlines of n bytes takes at most ceil((2113 + 15 n H + 15) / 8) + 4 <= 270 + ceil(15 n H / 8)
 *             bytes, and that is the bound everything sizes buffers with.
 *
 * ra_png_deflate_dyn_bound / ra_png_deflate_dyn_u8 / ra_png_deflate_dyn_host — the argument lists, kinds, plane list semantics,
 *   refusals and RA_E_* codes of their fixed counterparts above, with this format's bound.  On success the bytes of `out` outside
 *   the N streams are unspecified.  The workspace: per image a histogram (288 words) and a code table (1456 bytes), per row a
 *   16-byte record, an 8-byte place and a worst-case slot of ceil(15 n / 8) + 4 bytes rounded up to 16.
 *   The device entry: a stream-ordered clear of the histograms and five plain launches (histogram: a workgroup per scanline,
 *   32-bit integer atomic adds; code: one workgroup per image builds the lengths, the codes and the header bits; encode: a
 *   workgroup per scanline, token bits from the image's table in LDS — up to 70.2 KiB of LDS for the longest scanline; scan: a
 *   workgroup per image, 64-bit bit places; place: owner-computes per destination dword with a funnel shift, no atomics, nothing
 *   cleared), no allocation, no synchronisation, no workgroup waits for another.  The source is read twice.
 * ra_png_huffman_lengths — HOST code, no GPU call: THE RULE on counts[0 .. n), the function the code kernel runs.  limit 7 or 15
 *   (else RA_E_INVALID, as a NULL pointer), 1 <= n <= 286 and n <= 2^limit (else RA_E_SHAPE); lengths: n bytes.
 * ---------------------------------------------------------------------------------- */
int ra_png_deflate_dyn_bound(int N, int H, int W, int bpp, unsigned long long *stream_bytes, unsigned long long *workspace_bytes);
int ra_png_deflate_dyn_u8(const void *src, int kind, int M, int N, int H, int W, const int *plane, unsigned char *out,
                          size_t out_bytes, int *sizes, unsigned long long *offsets, unsigned int *adler, void *ws, size_t ws_bytes,
                          void *stream);
int ra_png_deflate_dyn_host(const void *src, int kind, int M, int N, int H, int W, const int *plane, unsigned char *out,
                            size_t out_bytes, int *sizes, unsigned long long *offsets, unsigned int *adler, void *ws,
                            size_t ws_bytes);
int ra_png_huffman_lengths(const unsigned int *counts, int n, int limit, unsigned char *lengths);

/* ------------------------------------------------------------------------------------
 * Evaluating the pre-stage fg_model (csrc/ra_fg_eval.hip).
 *
 * ra_fg_stats_f32 — the sums behind the six statistics the reference's Evaluator logs (fg_model_train.py:131-133), replacing
 *   the loss head of fg_model.py:196-248 at eval: logits [npix, nsc + no] (what ra_fg_head_f32 reads; the sigmoid / softmax
 *   are evaluated with its expressions, unquantised), y_gt [npix, nsc], d_gt [npix, no] (NULL when no == 0); nsc 1 .. 16,
 *   no 0 | 8.  sums: RA_FG_STAT_COUNT doubles —
 *     INTER_SOFT, SUM_SOFT, SUM_GT   sum y g, sum y, sum g of modellib.f_iou_all (modellib.py:171-181) over the foreground
 *                                    channels: the only channel for nsc == 1, channels 1 .. nsc - 1 otherwise (:208-218);
 *     INTER_HARD, SUM_HARD           the same with y replaced by hard = [logit > 0] (nsc == 1, :209) or [logit[c] == max_c
 *                                    logit] (:213-214; every maximum counts, as tf.equal does);
 *     SEG_CE                         sum f_bce(y, g) (nsc == 1) or sum f_ce(y, g) over ALL channels (:221-226,
 *                                    modellib.py:418-427), NOT yet divided by the pixel count;
 *     MASK                           sum m, m = g (nsc == 1) or max over c >= 1 of g[c] (:201-206); 0 when no == 0;
 *     ORI_CE, ORI_CORRECT            sum f_ce(d, d_gt) m and sum [argmax d_logit == argmax d_gt] m, first maximum on both
 *                                    sides (:235-246); 0 when no == 0.
 *   The hard quantities are taken on the LOGITS, not on rounded probabilities: equal in exact arithmetic, and float32
 *   rounding of a softmax must not invent ties.  float32 within a pixel, float64 and a fixed order from there on, no
 *   floating-point atomics: the same bits on every run.  ws: ra_fg_stats_workspace_bytes(npix) bytes, 8-byte aligned.
 * ra_fg_sweep_counts_f32 — the counters of analysis.py:834-906 (ForegroundIOUAnalyzer / BackgroundIOUAnalyzer) for every
 *   threshold of fg_model_eval.py:166-173 at once: src [N,Hs,Ws] the soft foreground at network size, gt uint8 [N,H,W] the
 *   full-size labels summed over the instances (:142-143; values above 1 where instances overlap count as a * b and b.sum()
 *   count them), thresholds: K floats in HOST memory, 1 <= K <= RA_FG_SWEEP_MAX_K.  With v = bilateralFilter(resize(src,
 *   (W, H)), 5, 10, 10) (:106-117; the arithmetic of ra_resize_linear_f32 + ra_bilateral5_f32, evaluated per tile and never
 *   written) counts [N, RA_FG_SWEEP_SLOTS] receives, per image, count_a[k] = #{v > thr[k]} at slot k, sum_ab[k] = sum of gt
 *   over those pixels at slot RA_FG_SWEEP_MAX_K + k, and sum_b = sum of gt at slot 2 RA_FG_SWEEP_MAX_K; slots of k >= K are
 *   0.  counts is cleared on the stream first; integer atomics, so the result does not depend on the order.  H * W < 2^31.
 * ---------------------------------------------------------------------------------- */
#define RA_FG_STAT_INTER_SOFT 0
#define RA_FG_STAT_SUM_SOFT 1
#define RA_FG_STAT_SUM_GT 2
#define RA_FG_STAT_INTER_HARD 3
#define RA_FG_STAT_SUM_HARD 4
#define RA_FG_STAT_SEG_CE 5
#define RA_FG_STAT_ORI_CE 6
#define RA_FG_STAT_ORI_CORRECT 7
#define RA_FG_STAT_MASK 8
#define RA_FG_STAT_COUNT 9
#define RA_FG_SWEEP_MAX_K 16
#define RA_FG_SWEEP_SLOTS 33
size_t ra_fg_stats_workspace_bytes(size_t npix);
int ra_fg_stats_f32(const float *logits, const float *y_gt, const float *d_gt, size_t npix, int nsc, int no, void *ws,
                    size_t ws_bytes, double *sums, void *stream);
int ra_fg_sweep_counts_f32(const float *src, const unsigned char *gt, int N, int Hs, int Ws, int H, int W,
                           const float *thresholds, int K, unsigned long long *counts, void *stream);

/* ------------------------------------------------------------------------------------
 * The decode loop's evaluator at the labels' size, from instance-id images (csrc/ra_instance_eval.hip).
 *
 * ra_instance_eval_counts_f32 — the reference's write_log chain behind apply_confidence (full_model_eval.py:112-124: upsample,
 *   postprocess.py:75-106; morph, :55-72; apply_one_label, :32-52; per threshold apply_threshold, :5-12, and mask_foreground,
 *   :139-147) reduced to the integers its analyzers read (analysis.py:314-787), for every threshold at once, in one pass that
 *   writes no [., Hf, Wf] plane.  yc [B,T,Hs,Ws]: y_out * s_out at network size (apply_confidence, :15-29, stays with the
 *   caller); gt_ids int32 [B,Hf,Wf] the instance-id image; inst_id int32 [B,T]: the id of ground-truth slot j, negative for
 *   an empty slot (what ra_labels_assemble_i32 at NETWORK size returns, so the slots keep the reference's order); fg uint8
 *   [B,Hf,Wf] or NULL, non-zero = foreground; morph: 0 | 1; thresholds: K floats in HOST memory, in any order.
 *   Per full-size pixel and t, v_t = bilateralFilter(resize(yc_t, (Wf, Hf)), 5, 10, 10) with the arithmetic of
 *   ra_resize_linear_f32 + ra_bilateral5_f32, with morph the maximum of that over the 5 x 5 window, pixels outside the image
 *   ignored (ra_dilate_f32).  The pixel goes to t* = the FIRST maximum over t, of value m; at threshold k it belongs to
 *   prediction t* iff m > thresholds[k] (and fg != 0 when fg is given); its ground-truth slot j is the first one with
 *   inst_id[b,j] equal to its id, T when there is none.  Outputs, exact integers: inter [B,K,T,T + 1] = the pixels of
 *   (prediction t*, slot j) at threshold k — column T holds the prediction's pixels on no listed instance, so a prediction's
 *   area is its row sum — and area_b [B,T] = the pixels of slot j.  Both are cleared on the stream first; integer atomics
 *   only, so two runs give the same bits.
 *   1 <= K <= RA_INS_EVAL_MAX_K, every threshold >= 0 (below zero the zeros of the planes that lost the arg-max would pass
 *   apply_threshold: another computation), 1 <= T <= RA_LABELS_MAX_T, Hf * Wf <= 2^24 (every count is then exact in the float32
 *   ra_eval_metrics_f32 takes), Hs * Ws < 2^31, B <= 65535: else RA_E_SHAPE before anything is launched.
 * ---------------------------------------------------------------------------------- */
#define RA_INS_EVAL_MAX_K 16
int ra_instance_eval_counts_f32(const float *yc, const int *gt_ids, const int *inst_id, const unsigned char *fg, int B, int T,
                                int Hs, int Ws, int Hf, int Wf, int morph, const float *thresholds, int K, int *inter,
                                int *area_b, void *stream);

/* ------------------------------------------------------------------------------------
 * Mixed full sizes in one batch (KITTI): the ragged forms of the four entry points that work at the labels' own size.
 *
 * A batch of B full-size images of different sizes is ONE flat buffer per per-pixel tensor (gt_ids int32, fg uint8,
 * fg_gt_full uint8, the sweep's gt uint8), all with the same geometry: image b is the h x w rows, packed with pitch w, that
 * start at element `offset` of the buffer (counted in elements, not bytes).  `total` is the buffer's element count.
 * Every entry takes the table twice: geo, B entries in HOST memory, checked before anything is launched or cleared, and
 * geo_dev, a caller-provided DEVICE buffer of B entries which the entry fills on the stream ahead of its kernels.  RA_E_SHAPE,
 * with a message that names the image, for: h < 1 or w < 1; an image that starts before the end of the one before it (the
 * table is in ascending order of offset; gaps are fine); an image that ends beyond `total`; an image that breaks a per-image
 * bound of the uniform entry point (h * w < 2^31; h * w <= 2^24 for ra_instance_eval_counts_ragged_f32; 1 <= H <= h and
 * 1 <= W <= w for ra_labels_assemble_ragged_i32).
 * Offsets need not be aligned.  The wide loads (16 bytes of ids, 4 bytes of uint8 labels per lane) are a PER-IMAGE decision,
 * made once per workgroup: they need w % 4 == 0, offset % 4 == 0 and base pointers aligned as the uniform forms want them; an
 * image that misses any of these takes element loads and its neighbours are unaffected.  The load width touches no arithmetic.
 * The kernels are the uniform forms' own, instantiated over the geometry source (csrc/ra_ragged.h): one table entry read per
 * workgroup into scalar registers; the grid's x extent follows the LARGEST image's tile count and a workgroup's loop bound is
 * its own image's, so one launch chain serves the batch.  Everything that is uniform in the batch stays a dense tensor: yc
 * [B,T,Hs,Ws], inst_id [B,T], src [N,Hs,Ws], the catalogue, the counts, the network-size labels [B,T,H,W] etc.
 *
 * ra_gt_instance_catalog_ragged_i32 — ra_gt_instance_catalog_i32 per image.  ws: ra_gt_instance_catalog_ragged_workspace_ints
 *   (geo, B) ints, sized from the largest image; the record of a workgroup whose image has fewer tiles than the grid is
 *   written empty, never left as it was.
 * ra_labels_assemble_ragged_i32 — ra_labels_assemble_i32 with the sampling scales sy, sx per image (the same double
 *   expressions, evaluated on the device once per workgroup); fg_gt_full is written flat at gt_ids' offsets (elements between
 *   images are not touched).  ws: ra_labels_workspace_bytes(B, H, W).
 * ra_instance_eval_counts_ragged_f32 — ra_instance_eval_counts_f32; gt_ids and fg (nullable) are flat, and the resize
 *   coordinates, reflect101, the in-image test of the dilation and the tile walk use the image's own h, w.
 * ra_fg_sweep_counts_ragged_f32 — ra_fg_sweep_counts_f32 with gt flat; counts [N, RA_FG_SWEEP_SLOTS] as there.
 * ---------------------------------------------------------------------------------- */
typedef struct ra_image_geo {
  long long offset;
  int h;
  int w;
} ra_image_geo;
size_t ra_gt_instance_catalog_ragged_workspace_ints(const ra_image_geo *geo, int B);
int ra_gt_instance_catalog_ragged_i32(const int *gt_ids, size_t total, const ra_image_geo *geo, ra_image_geo *geo_dev, int B,
                                      int *ws, size_t ws_ints, int *ids, int *pixels, int *count, int *status, void *stream);
int ra_labels_assemble_ragged_i32(const int *gt_ids, size_t total, const ra_image_geo *geo, ra_image_geo *geo_dev,
                                  const int *ids, const int *count, int B, int H, int W, int T, int dataset, void *ws,
                                  size_t ws_bytes, int *num_obj, float *s_gt, int *inst_id, int *area, int *sem_cls, float *y_gt,
                                  unsigned char *d_cls, float *d_gt, float *c_gt, unsigned char *fg_gt_full, void *stream);
int ra_instance_eval_counts_ragged_f32(const float *yc, const int *gt_ids, const int *inst_id, const unsigned char *fg,
                                       size_t total, const ra_image_geo *geo, ra_image_geo *geo_dev, int B, int T, int Hs, int Ws,
                                       int morph, const float *thresholds, int K, int *inter, int *area_b, void *stream);
int ra_fg_sweep_counts_ragged_f32(const float *src, const unsigned char *gt, size_t total, const ra_image_geo *geo,
                                  ra_image_geo *geo_dev, int N, int Hs, int Ws, const float *thresholds, int K,
                                  unsigned long long *counts, void *stream);

/* ------------------------------------------------------------------------------------
 * Pictures on the id path: the winner map out of the counting pass (csrc/ra_instance_eval.hip) and the kernels that paint from
 * it (csrc/ra_instance_paint.hip).  They replace, where the evaluator runs from instance-id images and no [B,T,Hf,Wf] mask
 * exists, analysis.py:137-147 (RenderInstanceAnalyzer), analysis.py:166-187 (RenderGroundtruthInstanceAnalyzer) and the masks
 * full_model_eval.py:65-79,139-140 hands them.
 *
 * ra_instance_eval_counts_map_f32 / ra_instance_eval_counts_map_ragged_f32 — ra_instance_eval_counts_f32 /
 *   ra_instance_eval_counts_ragged_f32, the same arguments and the same inter / area_b bit for bit, plus map: uint16 [B,Hf,Wf],
 *   or uint16 [total] flat at gt_ids' offsets (elements between the images are not written).  One word per pixel: n << 8 | t*,
 *   t* = the instance that holds the pixel's FIRST maximum m, n = how many of the call's thresholds, in ascending order, m
 *   exceeds with strict > (0 where fg masks the pixel); the whole word is 0 where n == 0, so the arg-max over values nobody
 *   reads is no part of the contract.  Threshold k AS GIVEN is passed iff n > pos[k].
 * ra_instance_eval_threshold_pos — pos[k] = how many of the K thresholds lie strictly below thresholds[k]: host arithmetic,
 *   the order the counting pass itself uses.  The checks on K and the thresholds are the counting pass's.
 * ra_instance_paint_u8 / ra_instance_paint_ragged_u8 — map as above; pos: Kp host ints, 1 <= Kp <= RA_INS_EVAL_MAX_K, each
 *   0 .. RA_INS_EVAL_MAX_K - 1; colour uint8 [B,Kp,T,3] in the memory order of the picture (B, G, R).  out: uint8
 *   [Kp,B,Hf,Wf,3], or [Kp,total,3] with image b of picture k from byte 3 * (k * total + offset_b) on.  A pixel of picture k
 *   is colour[b,k,t*] where n > pos[k], else 0 (also where t* >= T, which the counting pass never writes): the reference's
 *   sum over t of uint8(mask_t) * colour_t on disjoint masks.  remove_tiny is the caller's: a zeroed colour row.
 * ra_gt_paint_u8 / ra_gt_paint_ragged_u8 — gt_ids int32 [B,Hf,Wf] or [total]; inst_id int32 [B,T]; colour uint8 [B,T,3];
 *   out uint8 [B,Hf,Wf,3] or [total,3]: the colour of the first slot whose inst_id equals the pixel's id, 0 where no slot
 *   lists it or the id is negative — RA_RENDER_FIRST on the disjoint planes the id image defines, without the planes.
 * 1 <= T <= RA_LABELS_MAX_T, Hf * Wf (h * w) <= 2^24, B <= 65535, else RA_E_SHAPE; the ragged forms check the table as
 * every ragged entry does and name the image.  A lane's 4 pixels move as 8 (map) or 16 (ids) bytes in and 12 bytes out where
 * the image's first element and its pixel count are multiples of 4 (ragged: w % 4 == 0 and offset % 4 == 0) and the pointers
 * are aligned for it (picture k of a ragged batch also needs k * total % 4 == 0), per image; as elements and bytes otherwise.
 * ---------------------------------------------------------------------------------- */
int ra_instance_eval_counts_map_f32(const float *yc, const int *gt_ids, const int *inst_id, const unsigned char *fg, int B, int T,
                                    int Hs, int Ws, int Hf, int Wf, int morph, const float *thresholds, int K, int *inter,
                                    int *area_b, unsigned short *map, void *stream);
int ra_instance_eval_counts_map_ragged_f32(const float *yc, const int *gt_ids, const int *inst_id, const unsigned char *fg,
                                           size_t total, const ra_image_geo *geo, ra_image_geo *geo_dev, int B, int T, int Hs,
                                           int Ws, int morph, const float *thresholds, int K, int *inter, int *area_b,
                                           unsigned short *map, void *stream);
int ra_instance_eval_threshold_pos(const float *thresholds, int K, int *pos);
int ra_instance_paint_u8(const unsigned short *map, int B, int Hf, int Wf, const int *pos, int Kp, int T,
                         const unsigned char *colour, unsigned char *out, void *stream);
int ra_instance_paint_ragged_u8(const unsigned short *map, size_t total, const ra_image_geo *geo, ra_image_geo *geo_dev, int B,
                                const int *pos, int Kp, int T, const unsigned char *colour, unsigned char *out, void *stream);
int ra_gt_paint_u8(const int *gt_ids, const int *inst_id, int B, int T, int Hf, int Wf, const unsigned char *colour,
                   unsigned char *out, void *stream);
int ra_gt_paint_ragged_u8(const int *gt_ids, size_t total, const ra_image_geo *geo, ra_image_geo *geo_dev, const int *inst_id,
                          int B, int T, const unsigned char *colour, unsigned char *out, void *stream);

/* ------------------------------------------------------------------------------------
 * The device PNG encoder for a batch of MIXED sizes (KITTI): both stream formats above, unchanged — a stream is a function of
 * one image's scanlines alone, so every image gets the bytes a uniform call on it alone gives — in one launch chain for the
 * whole batch.  The kernels are the uniform entries' own, instantiated over the geometry source (csrc/ra_png_parts.h,
 * csrc/ra_ragged.h).  P is ra_png_deflate (fixed format) or ra_png_deflate_dyn (dynamic format).
 *
 * LAYOUT   src holds M planes of `total` elements each, all laid out by ONE table of B images (ra_image_geo, above: geo in
 *   HOST memory, checked before anything is launched, cleared or written; geo_dev a caller-provided DEVICE buffer of B entries,
 *   filled on the stream ahead of the kernels).  Image b of plane m is h_b rows of pitch w_b from element m * total + offset_b
 *   on.  An element is 1 byte (RA_PNG_GRAY8), 3 bytes in B, G, R order (RA_PNG_BGR8: what ra_instance_paint_ragged_u8 writes,
 *   [Kp,total,3]) or 4 bytes (RA_PNG_F32).
 * STREAMS  the call encodes N = Np * B streams; stream i = k * B + b is image b of plane plane[k], or of plane k when plane is
 *   NULL (then Np <= M).  The plane list has the semantics of the uniform entries: Np int32 in device memory, clamped in the
 *   kernel; the host entry refuses an index outside [0, M).  out, sizes [N], offsets [N], adler [N]: as in the uniform entries.
 * BOUNDS   P_ragged_bound — bpp 1 or 3.  *out_bytes = Np * the sum over b of the uniform entry's stream bound for h_b x w_b:
 *   what `out` must hold.  *workspace_bytes: the uniform entry's workspace for N images of Hmax = max h_b rows and scanlines of
 *   n_max = 1 + bpp * max w_b bytes.  Records, slots and bit places keep a uniform stride of Hmax (Hmax + 1) rows per stream,
 *   so no row-prefix table exists; the price is workspace sized by the tallest and the widest image of the batch (KITTI's four
 *   sizes, 370 x 1224 .. 376 x 1242: below 2 % more than the images need).
 * LAUNCHES the uniform chain's, three (fixed) or a clear and five (dynamic), whatever the mix of sizes.  The row grids are
 *   (Hmax, N); workgroup (r, i) reads table entry i % B — one scalar load — derives n and its threads' chunk from w_b and
 *   leaves before its first barrier when r >= h_b; the per-image loops of scan, compact and place are bounded by h_b.  LDS
 *   offsets are sized by n_max.  16-byte loads are decided per workgroup from the row's real address and width: the image's
 *   first byte 16-byte aligned and w_b * (source bytes per pixel) % 16 == 0; an image that misses takes element loads and its
 *   neighbours are unaffected (KITTI's widths miss: 1224 % 16 = 8).  No allocation, no synchronisation, no atomics beyond the
 *   histogram's, no workgroup waits for another.
 * P_ragged_host — HOST code, no GPU call: the same arguments in host memory without geo_dev and stream (ws may be NULL), the
 *   sequential rule image by image.  The same bytes as the device entry.
 * Refusals, before anything is read, written or launched; out, sizes, offsets and adler stay untouched: a NULL src, geo,
 *   geo_dev, out, sizes, offsets or adler, or another kind: RA_E_INVALID.  M < 1, N < 1 or N > RA_PNG_MAX_IMAGES, Np > M without a
 *   plane list: RA_E_SHAPE.  A table that breaks the rules of every ragged entry (h, w >= 1, ascending, no overlap, inside
 *   `total`), or an image whose scanline exceeds RA_PNG_MAX_ROW_BYTES, whose source holds 2^31 bytes or whose stream bound
 *   reaches 2^31: RA_E_SHAPE, the message names the image.  out_bytes below the bound, a NULL, short or not 16-byte aligned ws
 *   (device entry): RA_E_WORKSPACE.
 * ---------------------------------------------------------------------------------- */
int ra_png_deflate_ragged_bound(const ra_image_geo *geo, int B, int Np, int bpp, unsigned long long *out_bytes,
                                unsigned long long *workspace_bytes);
int ra_png_deflate_ragged_u8(const void *src, int kind, int M, size_t total, const ra_image_geo *geo, ra_image_geo *geo_dev, int B,
                             const int *plane, int Np, unsigned char *out, size_t out_bytes, int *sizes,
                             unsigned long long *offsets, unsigned int *adler, void *ws, size_t ws_bytes, void *stream);
int ra_png_deflate_ragged_host(const void *src, int kind, int M, size_t total, const ra_image_geo *geo, int B, const int *plane,
                               int Np, unsigned char *out, size_t out_bytes, int *sizes, unsigned long long *offsets,
                               unsigned int *adler, void *ws, size_t ws_bytes);
int ra_png_deflate_dyn_ragged_bound(const ra_image_geo *geo, int B, int Np, int bpp, unsigned long long *out_bytes,
                                    unsigned long long *workspace_bytes);
int ra_png_deflate_dyn_ragged_u8(const void *src, int kind, int M, size_t total, const ra_image_geo *geo, ra_image_geo *geo_dev,
                                 int B, const int *plane, int Np, unsigned char *out, size_t out_bytes, int *sizes,
                                 unsigned long long *offsets, unsigned int *adler, void *ws, size_t ws_bytes, void *stream);
int ra_png_deflate_dyn_ragged_host(const void *src, int kind, int M, size_t total, const ra_image_geo *geo, int B, const int *plane,
                                   int Np, unsigned char *out, size_t out_bytes, int *sizes, unsigned long long *offsets,
                                   unsigned int *adler, void *ws, size_t ws_bytes);

/* ------------------------------------------------------------------------------------
 * Training the pre-stage fg_model (csrc/ra_fg_loss.hip).
 *
 * ra_fg_loss_bwd_f32 — the gradient of the loss head of fg_model.py:196-248 with respect to the logits [npix, nsc + no]; the
 *   forward value is ra_fg_stats_f32.  y_gt [npix, nsc], d_gt [npix, no] (NULL when no == 0), nsc 1 .. 16, no 0 | 8,
 *   segm_loss_fn 0 = iou (loss = -I / U over the whole batch, modellib.py:171-181) | 1 = bce (f_bce for nsc == 1, f_ce over all
 *   channels otherwise, divided by npix; :221-233).  sums: the RA_FG_STAT_COUNT device doubles ra_fg_stats_f32 wrote for the
 *   same tensors, read on the device (no host synchronisation).  upstream: dL/dloss.  With p = sigmoid(z) (nsc == 1) or
 *   softmax(z[0:nsc]), evaluated with the expressions of ra_fg_head_f32, and eps = 1e-5 kept inside the logarithms
 *   (modellib.py:418-427), so that the derivative is of log(p + eps):
 *     bce   q = (-g / (p + eps) + (1 - g) / (1 - p + eps)) / npix        (nsc == 1);  q_c = -g_c / (p_c + eps) / npix  (nsc > 1)
 *     iou   q = -(g U - I (1 - g)) / U^2, U = sum p + sum g - I + 1e-5; for nsc > 1 over the channels c >= 1, q_0 = 0 (:215)
 *     dz = q p (1 - p)  (nsc == 1);   dz_c = p_c (q_c - sum_j p_j q_j)  (nsc > 1)
 *   and for no == 8, with m = g (nsc == 1) or max over c >= 1 of g_c (:201-206), d = softmax(z[nsc:]), MASK = sum m:
 *     q_k = -d_gt_k m / (d_k + eps) / MASK, then the same softmax adjoint (:235-240).
 *   orientation_acc and the hard IoU carry no gradient.  When no == 8 and MASK == 0 the reference divides 0 by 0 and trains on
 *   NaN; here the orientation logits' gradient is written as 0 and status[0] = 1 (else status[0] = 0), for the guarded
 *   optimizer entries to skip the step.  dlogits [npix, nsc + no]; no floating-point atomics: the same bits on every run.
 * ra_momentum_step_guarded_f32 — tf.train.MomentumOptimizer(lr, momentum) on one flat float32 bucket of n parameters
 *   (fg_model.py:262-263): g = grads * grad_scale + wd_coef * params (wd_coef nullable), accum = momentum * accum + g,
 *   params -= lr * accum; applied ONLY IF none of the n_status device words is non-zero (status nullable with n_status 0), the
 *   contract of ra_adam_step_guarded_f32's n_other words.
 * ---------------------------------------------------------------------------------- */
int ra_fg_loss_bwd_f32(const float *logits, const float *y_gt, const float *d_gt, size_t npix, int nsc, int no,
                       int segm_loss_fn, const double *sums, float upstream, float *dlogits, int *status, void *stream);
int ra_momentum_step_guarded_f32(float *params, const float *grads, float *accum, const float *wd_coef, size_t n, float lr,
                                 float momentum, float grad_scale, const int *status, int n_status, void *stream);

/* ------------------------------------------------------------------------------------
 * Training step (full_model.py:1039-1057).
 * ra_adam_step_f32 — gradient clip + Adam on one flat float32 bucket of n parameters:
 *   g = clip(grads * grad_scale + wd_coef * params, -clip, clip)   (wd_coef nullable; the
 *       wd * l2_loss(w) terms of nnlib.py:59-61 belong to total_loss; grad_scale = 1 / world
 *       after the data-parallel RCCL sum),
 *   m, v, params updated as tf.train.AdamOptimizer does (epsilon outside the bias correction);
 *   lr_t = learn_rate * sqrt(1 - beta2^t) / (1 - beta1^t) is computed by the caller.
 * ---------------------------------------------------------------------------------- */
int ra_adam_step_f32(float *params, const float *grads, float *m, float *v, const float *wd_coef,
                     size_t n, float lr_t, float beta1, float beta2, float eps, float clip,
                     float grad_scale, void *stream);
/* The same update, applied ONLY IF none of the step's device status words says "failed": the first n_solver words are
 * Hungarian-solver return codes (negative = the reference's LOG(FATAL) cases, hungarian.cc:126,148,158,187,448; 1 = the
 * outer cap, where the reference carries on with the partial matching, :363-377 — not a failure), the n_other words behind
 * them fail when non-zero (the split controller's time-out word, another rank's failure flag).  A training loop that reads
 * those words one step late (no host sync per step) can then never have applied a failed step's gradients.  status
 * nullable with both counts 0 (= ra_adam_step_f32). */
int ra_adam_step_guarded_f32(float *params, const float *grads, float *m, float *v, const float *wd_coef,
                             size_t n, float lr_t, float beta1, float beta2, float eps, float clip,
                             float grad_scale, const int *status, int n_solver, int n_other, void *stream);

/* Train-mode layer pieces of nnlib.cnn / nnlib.dcnn (nnlib.py:229-253,362-400 with
 * phase_train = True).  The convolution itself is ra_conv3x3_f32 with scale = 1, shift = bias,
 * no ReLU, no pool (u = conv(x, w) + b); then
 *   ra_bn_moments_f32       mean[c], var[c] = tf.nn.moments(u, [0,1,2]) (nnlib.py:98; biased,
 *                           two passes, fixed summation order); u [npix, C], C <= 256.
 *   ra_bn_act_pool_f32      y = max_pool(relu?(gamma (u - mean) rsqrt(var + eps) + beta))
 *                           (nnlib.py:111-119,250-253); mean/var/gamma/beta nullable together
 *                           (use_bn False: y = pool(relu(u))).
 *   ra_bn_act_pool_bwd_f32  given dy [B,H/pool,W/pool,C]: dbeta, dgamma [C] and
 *                           du = gamma rstd (dv - mean(dv) - xhat mean(dv xhat)), dv = dy routed to
 *                           the first maximum of each pool window and masked by the ReLU — the
 *                           batch statistics are differentiated through, as tf.gradients does.
 *   ws: ra_bn_workspace_floats(C) device floats.
 * ra_conv_pack_weights_dev  ra_conv_pack_weights on device pointers (weights change every step).
 * ra_conv3x3_wgrad_f32      dWf[ky][kx][ci][co] = sum X[b,y+ky-1,x+kx-1,ci] dU[b,y,x,co] for the
 *                           SAME conv that ran (X zero-stuffed when upsample = 1), db[co] = sum dU
 *                           (db nullable); f32 MFMA with pixels as the K dimension; Cout <= 64;
 *                           ws: ra_conv3x3_wgrad_workspace_floats() floats.
 *   Backward-data is ra_conv3x3_f32 itself on the flipped / in-out-swapped packing
 *   (RA_CONV_TRANSPOSED for a cnn layer, plain packing of the [3,3,out,in] filter for a dcnn
 *   layer), followed for stride-2 layers by
 * ra_subsample_odd_f32      y[b,i,j,:] = x[b,2i+1,2j+1,:], x [B,2H,2W,C] (adjoint of zero-stuffing).
 * ra_weighted_sum_multi_f32 out[b,n,:] = sum_t w[b,n,t] y[b,t,:] + bias[b,n]: with the coefficients
 *                           of modellib.f_iou's quotient rule this is d loss / d y_out. */
size_t ra_bn_workspace_floats(int C);
int ra_bn_moments_f32(const float *u, size_t npix, int C, float *ws, size_t ws_floats, float *mean,
                      float *var, void *stream);
int ra_bn_act_pool_f32(const float *u, const float *mean, const float *var, const float *gamma,
                       const float *beta, float eps, int relu, int pool, int B, int H, int W, int C,
                       float *y, void *stream);
int ra_bn_act_pool_bwd_f32(const float *u, const float *dy, const float *mean, const float *var,
                           const float *gamma, const float *beta, float eps, int relu, int pool,
                           int B, int H, int W, int C, float *ws, size_t ws_floats, float *dgamma,
                           float *dbeta, float *du, void *stream);
int ra_conv_pack_weights_dev(const float *w, int Cin_w, int Cout, int Cin, const int *chan_map,
                             int flags, float *out, void *stream);
size_t ra_conv3x3_wgrad_workspace_floats(int Cin, int Cout, int B, int H, int W);
int ra_conv3x3_wgrad_f32(const float *x, int Cin, int B, int Hs, int Ws, int upsample,
                         const float *du, int Cout, float *ws, size_t ws_floats, float *dw,
                         float *db, void *stream);
/* The accumulating forms add the layer's parameter gradients straight into the trainer's flat
 * gradient bucket (one writer per element), replacing ~2 500 small `grad += g` launches of a step:
 *   ra_conv3x3_wgrad_acc_f32    gw += dW in the REFERENCE layout of the filter that ran — [3,3,cin_w,Cout],
 *                               or [3,3,Cout,cin_w] with flipped taps when transposed (nnlib.dcnn's
 *                               filters, nnlib.py:362-400) — chan_map (device, nullable) sends packed kernel
 *                               channel c to filter row chan_map[c] (-1: padding); gb += db (nullable).
 *   ra_bn_act_pool_bwd_acc_f32  ra_bn_act_pool_bwd_f32 + acc_gamma += dgamma, acc_beta += dbeta (nullable). */
int ra_conv3x3_wgrad_acc_f32(const float *x, int Cin, int B, int Hs, int Ws, int upsample,
                             const float *du, int Cout, float *ws, size_t ws_floats, const int *chan_map,
                             int cin_w, int transposed, float *gw, float *gb, void *stream);
/* The filter gradient with bf16 operands (x and du rounded to bf16 from LDS, float32 accumulation over the pixels
 * and float32 partial sums): the mixed-precision counterparts of the two entries above. */
int ra_conv3x3_wgrad_bf16ops_f32(const float *x, int Cin, int B, int Hs, int Ws, int upsample,
                                 const float *du, int Cout, float *ws, size_t ws_floats, float *dw,
                                 float *db, void *stream);
int ra_conv3x3_wgrad_acc_bf16ops_f32(const float *x, int Cin, int B, int Hs, int Ws, int upsample,
                                     const float *du, int Cout, float *ws, size_t ws_floats,
                                     const int *chan_map, int cin_w, int transposed, float *gw, float *gb,
                                     void *stream);
/* A layer whose filter is shared by the T timesteps of a training step (every nnlib.cnn / dcnn layer of full_model:
 * one set of weights, full_model.py:455-535) sums its T filter gradients — in ONE pass over the images of all T calls: ra_conv3x3_wgrad_multi_acc_f32 is ra_conv3x3_wgrad_acc_f32 on
 * nseg * Bseg images read through two device tables of nseg pointers (x [Bseg,Hs,Ws,Cin] and du [Bseg,H,W,Cout] of
 * each call; workspace for B = nseg * Bseg).  ra_ptr_table writes up to 64 device pointers given as a HOST array into
 * a device table by a kernel launch, so that the tables can be built inside a captured HIP graph. */
int ra_ptr_table(const void *const *host_ptrs, int n, void **dev_table, void *stream);
int ra_conv3x3_wgrad_multi_acc_f32(const void *const *xtab, const void *const *dutab, int nseg, int Cin, int Bseg,
                                   int Hs, int Ws, int upsample, int Cout, float *ws, size_t ws_floats,
                                   const int *chan_map, int cin_w, int transposed, float *gw, float *gb,
                                   int bf16_operands, void *stream);
/* Training nnlib.cnn / nnlib.dcnn layers of filter size KF in {1, 5, 7} (nnlib.py:131-257, :260-404; csrc/ra_wgrad_kxk.hip).
 * ra_convkxk_wgrad_f32 / _acc_f32: ra_conv3x3_wgrad_f32 / _acc_f32 with KF taps, for the SAME conv ra_convkxk_f32 ran:
 *   dW[ky][kx][ci][co] = sum_{b,y,x} X[b,y+ky-p,x+kx-p,ci] dU[b,y,x,co], db[co] = sum dU; X zero-padded, p = KF / 2; with
 *   upsample X is the zero-stuffed image of the stride-2 transposed conv under the forward's window for that KF.  dw
 *   [KF,KF,Cin,Cout]; the accumulate entry adds to gw in the reference layout ([KF,KF,Cin_w,Cout], or transposed: taps
 *   flipped, [KF,KF,Cout,Cin_w]; chan_map: device, nullable) and to gb (nullable).  f32 MFMA, the taps' rows split over the
 *   grid, per-workgroup partial records and a fixed-order finishing launch: no atomics, two runs give the same bits.  The
 *   caller owns ws (ra_convkxk_wgrad_workspace_floats(KF, Cin, Cout, B, H, W) floats, H, W = the conv's map: twice x's with
 *   upsample); nothing is allocated or synchronised.  KF = 3 forwards to the 3x3 entries; another KF, Cin % 4 != 0 or
 *   Cout > 128 return RA_E_SHAPE (the workspace query: 0) without a launch.
 * ra_convkxk_wgrad_plan: the chooser's answer for KF in {1, 5, 7} (host only, launches nothing): rec receives
 *   RA_WGK_PLAN_INTS ints indexed by RA_WGK_PLAN_*.  The one variable of the launch form is NT, the 16-channel tiles of Cout
 *   per workgroup: 1 for Cout <= 16, else 2.
 * ra_conv_pack_weights_k_dev: ra_conv_pack_weights_k on device pointers (weights change every step).
 * ra_subsample_even_f32: y[b,i,j,:] = x[b,2i,2j,:], x [B,2H,2W,C]: the data gradient of a stride-2 transposed layer of
 *   filter size 1 (dx[i] = du[2i] w; the centred windows of KF = 3, 5, 7 sit on 2i + 1: ra_subsample_odd_f32). */
#define RA_WGK_PLAN_INTS 8
#define RA_WGK_PLAN_NT 0
#define RA_WGK_PLAN_GRID_X 1
#define RA_WGK_PLAN_GRID_Y 2
#define RA_WGK_PLAN_GRID_Z 3
#define RA_WGK_PLAN_LDS_BYTES 4
#define RA_WGK_PLAN_RECORD_FLOATS 5
#define RA_WGK_PLAN_NTILES 6
#define RA_WGK_PLAN_ACC_TILES 7
size_t ra_convkxk_wgrad_workspace_floats(int KF, int Cin, int Cout, int B, int H, int W);
int ra_convkxk_wgrad_plan(int KF, int Cin, int Cout, int B, int H, int W, int *rec);
int ra_convkxk_wgrad_f32(const float *x, int Cin, int B, int Hs, int Ws, int upsample, const float *du, int Cout, int KF,
                         float *ws, size_t ws_floats, float *dw, float *db, void *stream);
int ra_convkxk_wgrad_acc_f32(const float *x, int Cin, int B, int Hs, int Ws, int upsample, const float *du, int Cout, int KF,
                             float *ws, size_t ws_floats, const int *chan_map, int Cin_w, int transposed, float *gw, float *gb,
                             void *stream);
int ra_conv_pack_weights_k_dev(const float *w, int KF, int Cin_w, int Cout, int Cin, const int *chan_map, int flags, float *out,
                               void *stream);
int ra_subsample_even_f32(const float *x, int B, int H, int W, int C, float *y, void *stream);
int ra_bn_act_pool_bwd_acc_f32(const float *u, const float *dy, const float *mean, const float *var,
                               const float *gamma, const float *beta, float eps, int relu, int pool,
                               int B, int H, int W, int C, float *ws, size_t ws_floats, float *dgamma,
                               float *dbeta, float *du, float *acc_gamma, float *acc_beta, void *stream);
/* G calls of one layer (its G timesteps: per-timestep statistics and parameters, nnlib.py:121-127) stacked along the
 * batch and differentiated in one reduce / final / dx triple: u [G*B,H,W,C], dy [G*B,H/pool,W/pool,C], du like u;
 * tabs = a DEVICE table of 6 G pointers {mean, var, gamma, beta, gradient-bucket gamma, gradient-bucket beta}[G]
 * (the last two are added to); dgamma / dbeta [G,C]; ws of G * ra_bn_workspace_floats(C) floats.  Where ra_bn_form
 * reports no form for the grouped call it returns RA_E_SHAPE without a launch: call the per-group entry. */
int ra_bn_act_pool_bwd_grouped_f32(const float *u, const float *dy, const void *const *tabs, int G, float eps,
                                   int relu, int pool, int B, int H, int W, int C, float *ws, size_t ws_floats,
                                   float *dgamma, float *dbeta, float *du, void *stream);
/* The same backward in two launches groups, for data-parallel training on WHOLE-batch statistics (nnlib.py:98
 * takes the moments over the whole batch): _reduce writes this rank's sums dbeta / dgamma (and adds them to
 * acc_*, may be NULL); the caller all-reduces the 2C sums; _dx finishes with the summed vectors and the
 * global pixel count n_total (mean / var are then the whole-batch moments too). */
int ra_bn_act_pool_bwd_reduce_f32(const float *u, const float *dy, const float *mean, const float *var,
                                  const float *gamma, const float *beta, float eps, int relu, int pool, int B, int H,
                                  int W, int C, float *ws, size_t ws_floats, float *dgamma, float *dbeta,
                                  float *acc_gamma, float *acc_beta, void *stream);
int ra_bn_act_pool_bwd_dx_f32(const float *u, const float *dy, const float *mean, const float *var,
                              const float *gamma, const float *beta, const float *dgamma_sum, const float *dbeta_sum,
                              double n_total, float eps, int relu, int pool, int B, int H, int W, int C, float *du,
                              void *stream);
/* The kernel form a BatchNorm pass runs at a shape: the one host function every ra_bn_* entry point asks.  Host only, launches
 * nothing.  pass: RA_BN_PASS_*; u [B,H,W,C] (moments: npix = B H W; pool is ignored); flags: the bf16 storage bits of the
 * *_bf16_f32 entry points, 0 for float32 tensors; stages (per-call backward): 1 = _reduce, 2 = _dx, 3 = both in one call;
 * G: 0 = a per-call backward, > 0 = ra_bn_act_pool_bwd_grouped_* over G groups.  Returns RA_BN_FORM_SMALL (the whole call in
 * one workgroup), RA_BN_FORM_V4 (four channels per thread; the only form that takes bf16 storage) or RA_BN_FORM_GENERIC, or
 * the RA_E_* code with which the entry point would refuse the call. */
#define RA_BN_PASS_MOMENTS 0
#define RA_BN_PASS_FORWARD 1
#define RA_BN_PASS_BACKWARD 2
#define RA_BN_FORM_SMALL 1
#define RA_BN_FORM_V4 2
#define RA_BN_FORM_GENERIC 3
int ra_bn_form(int pass, int C, int B, int H, int W, int pool, int flags, int stages, int G);
/* Training the WIDE layers of fg_model (fg_model.py:112-160 trained by :249-265; nnlib.cnn nnlib.py:229-253 and nnlib.dcnn
 * nnlib.py:362-400 with phase_train = True): the train-mode pieces above for the channel counts K1-wide runs, Cout 129 .. 512
 * (a multiple of 16) and Cin <= 1024 (a multiple of 4) = ra_conv_wide_supported(Cin, Cout).  Float32 storage only.  The
 * forward is ra_conv3x3_wide_f32 with scale = 1, shift = bias, no ReLU, no pool; its data gradient is the same kernel on the
 * flipped, in/out-swapped packing.  New entries beside the narrow ones: none of those changes what it answers.
 *   ra_conv_wide_pack_weights_dev  ra_conv_wide_pack_weights on DEVICE pointers (weights change every step), restricted to the
 *                                  output channels [co_first, co_first + co_count) of the filter: out = the host pack of that
 *                                  slice, bit for bit, ra_conv_wide_packed_floats(Cin, co_count) floats; co_count obeys
 *                                  the wide range.  A data gradient of more than 512 channels is two ranges.  chan_map: device,
 *                                  nullable; an entry outside [0, Cin_w) packs zeros.
 *   ra_conv3x3_wgrad_wide_acc_f32  ra_conv3x3_wgrad_acc_f32 for the wide range (csrc/ra_wgrad_wide.hip): gw += dW in the reference
 *                                  layout of the filter that ran, gb += db (nullable), one writer per element, no atomics,
 *                                  fixed order.  Output-stationary on v_mfma_f32_16x16x4_f32, the pixels (K) split over
 *                                  workgroups and summed by a second pass.  ws: ra_conv3x3_wgrad_wide_workspace_floats(Cin,
 *                                  Cout, B, H, W) floats, H, W = the conv's map (twice x's with upsample).
 *   ra_conv3x3_wgrad_wide_plan     the one chooser's answer for x [B,H,W,Cin] (host only, launches nothing): rec receives
 *                                  RA_WGW_PLAN_INTS ints, indexed by RA_WGW_PLAN_*: the workgroup's ci x co block and pixel tile
 *                                  side, taps per workgroup, grid (ci blocks, co blocks, K split), pixel tiles per part and in
 *                                  all, static LDS bytes, workspace floats.  RA_E_SHAPE where the launch would refuse.
 *   ra_bn_wide_*                   nnlib.py:98-119,250-253 as ra_bn_moments_f32 / ra_bn_act_pool_f32 /
 *                                  ra_bn_act_pool_bwd_acc_f32 with the same arithmetic, for any C % 4 == 0, C <= 512
 *                                  (csrc/ra_bn_wide.hip: a thread owns a channel quad of one pooling window, C / 4 need not be
 *                                  a power of two); ws: ra_bn_wide_workspace_floats(C) floats.  Else RA_E_SHAPE, no launch. */
#define RA_WGW_PLAN_INTS 12
#define RA_WGW_PLAN_TILE_CI 0
#define RA_WGW_PLAN_TILE_CO 1
#define RA_WGW_PLAN_TILE_PIX 2
#define RA_WGW_PLAN_TAPS 3
#define RA_WGW_PLAN_GRID_CI 4
#define RA_WGW_PLAN_GRID_CO 5
#define RA_WGW_PLAN_SPLIT 6
#define RA_WGW_PLAN_TILES_PER_PART 7
#define RA_WGW_PLAN_NTILES 8
#define RA_WGW_PLAN_LDS 9
#define RA_WGW_PLAN_WS_FLOATS 10
int ra_conv_wide_pack_weights_dev(const float *w, int Cin_w, int Cout, int Cin, const int *chan_map, int flags, int co_first,
                                  int co_count, float *out, void *stream);
size_t ra_conv3x3_wgrad_wide_workspace_floats(int Cin, int Cout, int B, int H, int W);
int ra_conv3x3_wgrad_wide_acc_f32(const float *x, int Cin, int B, int Hs, int Ws, int upsample, const float *du, int Cout,
                                  float *ws, size_t ws_floats, const int *chan_map, int cin_w, int transposed, float *gw,
                                  float *gb, void *stream);
int ra_conv3x3_wgrad_wide_plan(int Cin, int Cout, int B, int H, int W, int upsample, int *rec);
size_t ra_bn_wide_workspace_floats(int C);
int ra_bn_wide_moments_f32(const float *u, size_t npix, int C, float *ws, size_t ws_floats, float *mean, float *var,
                           void *stream);
int ra_bn_wide_act_pool_f32(const float *u, const float *mean, const float *var, const float *gamma, const float *beta,
                            float eps, int relu, int pool, int B, int H, int W, int C, float *y, void *stream);
int ra_bn_wide_act_pool_bwd_acc_f32(const float *u, const float *dy, const float *mean, const float *var, const float *gamma,
                                    const float *beta, float eps, int relu, int pool, int B, int H, int W, int C, float *ws,
                                    size_t ws_floats, float *dgamma, float *dbeta, float *du, float *acc_gamma,
                                    float *acc_beta, void *stream);
/* The pointwise half of the controller's LSTM cell (nnlib.py:641-646; the GEMM half is a library call):
 * pre [B][4*hid] = gate pre-activations in the order (i, f, o, u), c_prev [B][hid]:
 *   c = sigm(f) c_prev + sigm(i) tanh(u),  h = sigm(o) tanh(c);  act [B][4*hid] keeps the gate values.
 * Backward: dh / dc nullable (a gradient that does not exist is zero) -> dpre [B][4*hid], dc_prev. */
int ra_lstm_cell_f32(const float *pre, const float *c_prev, int B, int hid, float *h, float *c,
                     float *act, void *stream);
int ra_lstm_cell_bwd_f32(const float *act, const float *c_prev, const float *c, const float *dh,
                         const float *dc, int B, int hid, float *dpre, float *dc_prev, void *stream);
/* modellib.get_gaussian_filter (modellib.py:581-612) and its adjoint for the training graph:
 *   out[b][l][j] = N(l; mu_j, exp(lg_var[b])),  mu_j = ctr[b] + (size[b] + 1) / NF * (j - (NF - 1) / 2);
 *   backward: g [B][L][NF] -> dctr, dsize, dlg_var [B] (the bank is recomputed, not stored). */
int ra_gauss_filter_f32(const float *ctr, const float *size, const float *lg_var, int B, int L, int NF,
                        float *out, void *stream);
int ra_gauss_filter_bwd_f32(const float *ctr, const float *size, const float *lg_var, const float *g,
                            int B, int L, int NF, float *dctr, float *dsize, float *dlg_var,
                            void *stream);
/* The same two with element strides between consecutive images (one column of a [B,2] tensor is handed in
 * as it lies; stride_lg_var may be 0: one variance for all images); stride_grad: of dctr / dsize / dlg_var. */
int ra_gauss_filter_strided_f32(const float *ctr, const float *size, const float *lg_var, int stride_ctr,
                                int stride_size, int stride_lg_var, int B, int L, int NF, float *out,
                                void *stream);
int ra_gauss_filter_strided_bwd_f32(const float *ctr, const float *size, const float *lg_var,
                                    int stride_ctr, int stride_size, int stride_lg_var, const float *g,
                                    int B, int L, int NF, float *dctr, float *dsize, float *dlg_var,
                                    int stride_grad, void *stream);
/* The scalar head of the training loss with box_loss_fn = segm_loss_fn = 'iou' (full_model.py:913-1035) in one launch each
 * way.  iou_s / iou_b: the pairwise soft IoU of the masks / attention boxes against the ground truth [B,T,T] (pred, gt);
 * m_s / m_b: their matchings (f_segm_match); s_out [B,T]: the scores.
 *   ra_loss_head_f32      pieces[0..5] = loss, box_loss, segm_loss, conf_loss, iou_soft, iou_soft_box, where
 *                         iou = mean_b sum(iou * m) / max(sum m, 1), conf = sum(-ms log(cummin s + 1e-5) - (1 - ms)
 *                         log(1 - reverse-cummax s + 1e-5)) / B / T with ms = sum_gt m_s, loss = -iou_box - iou_soft +
 *                         mix * conf.
 *   ra_loss_head_bwd_f32  g (device scalar, NULL = 1): d loss upstream.  Writes the coefficients of the two pairwise-IoU
 *                         adjoints, c1 [B,T,T] / c0 [B,T] for ra_weighted_sum_multi_f32 (from inter / sum_a / sum_b of
 *                         ra_pair_stats_f32, HW = pixels per plane), and d s_out [B,T] (the cumulative extrema route their
 *                         gradient to the positions torch.cummin / cummax report on the CPU: among equal scores the LAST
 *                         position of the running minimum, and the smallest index >= t holding the maximum of s[t..T)).
 *   B <= 256, T <= 64, else RA_E_SHAPE and nothing is launched. */
int ra_loss_head_f32(const float *iou_s, const float *iou_b, const float *m_s, const float *m_b, const float *s_out, int B, int T,
                     float mix, float *pieces, void *stream);
int ra_loss_head_bwd_f32(const float *g, const float *m_s, const float *m_b, const float *s_out, const float *inter_s,
                         const float *sum_a_s, const float *sum_b_s, const float *inter_b, const float *sum_a_b,
                         const float *sum_b_b, int B, int T, int HW, float mix, float *c1_s, float *c0_s, float *c1_b,
                         float *c0_b, float *d_s_out, void *stream);
/* The attention head of the training graph in one launch each way (it is scalar math on nine numbers per image):
 *   ra_attn_head_f32   ctrl_out [B][stride >= 9] -> out [B][16] = cn[2] ls[2] ctr[2] size[2] lg_var[2] attn_gamma
 *                      box_gamma y_lg_gamma (full_model.py:702-722, modellib.py:752-764,812-825); flags: 1 squash
 *                      (tanh / -softplus), 2 fixed_var, 4 dynamic_var, 8 fixed_gamma.
 *   ra_attn_head_bwd_f32  gradients of those fields (dense [B,2] / [B], each nullable = zero) -> d ctrl_out [B][9].
 *   ra_knob_mix_f32    the ground-truth knob on the window (full_model.py:744-773): p2 = knob m + (1 - knob) p for
 *                      centre and size, m = sum_t match[b][t] gt[b][t][:]; knob [B] with element stride knob_stride,
 *                      ctr / size rows row_stride floats apart (fields of the head's record); outputs dense [B,2].
 *   ra_knob_mix_bwd_f32   d p = (1 - knob) g (g nullable).
 *   ra_attn_head_rec_f32 / ra_knob_mix_rec_f32   the same, also writing the window as the resample kernels' attention
 *                      record [B][RA_ATTN_STRIDE] (ctr, size, lg_var, attn_gamma, box_gamma, y_lg_gamma, zeros; the knob
 *                      form copies attn_rec with the mixed centre and size): every resample kernel reads only its own
 *                      gamma column, so ONE record serves the box, the extract and the paste of a timestep. */
int ra_attn_head_f32(const float *ctrl_out, int stride, int B, int H, int W, int Fh, int Fw, int flags,
                     float *out, void *stream);
int ra_attn_head_bwd_f32(const float *ctrl_out, int stride, const float *out, const float *g_cn,
                         const float *g_ls, const float *g_ctr, const float *g_size, const float *g_lg_var,
                         const float *g_attn_gamma, const float *g_box_gamma, const float *g_y_lg_gamma, int B,
                         int H, int W, int flags, float *d_ctrl_out, void *stream);
int ra_knob_mix_f32(const float *ctr, const float *size, const float *match, const float *ctr_gt,
                    const float *size_gt, const float *knob, int knob_stride, int row_stride, int B, int T,
                    float *ctr2, float *size2, void *stream);
int ra_knob_mix_bwd_f32(const float *g_ctr2, const float *g_size2, const float *knob, int knob_stride, int B,
                        float *d_ctr, float *d_size, void *stream);
int ra_attn_head_rec_f32(const float *ctrl_out, int stride, int B, int H, int W, int Fh, int Fw, int flags,
                         float *out, float *attn_rec, void *stream);
int ra_knob_mix_rec_f32(const float *ctr, const float *size, const float *match, const float *ctr_gt,
                        const float *size_gt, const float *knob, int knob_stride, int row_stride, int B, int T,
                        float *ctr2, float *size2, const float *attn_rec, float *attn_rec2, void *stream);
int ra_subsample_odd_f32(const float *x, int B, int H, int W, int C, float *y, void *stream);
/* The canvas update of a training timestep (full_model.py:826-848, stop_canvas_grad) and the next timestep's packed
 * controller-CNN input in one launch: inp_next = inp_prev [B,HW,C] with channel canvas_chan replaced by
 * max(y_c, canvas), y_c = y [B,HW], or with the ground-truth knob (match [B,T] != NULL)
 * knob[b] * (g - g * noise) + (1 - knob[b]) * y,  g = sum_t match[b,t] y_gt[b,t,:]  (noise [B,HW] nullable;
 * knob read at stride knob_stride).  No gradient flows through it. */
int ra_canvas_step_f32(const float *inp_prev, int C, int canvas_chan, int B, int HW, const float *y,
                       const float *match, const float *y_gt, int T, const float *noise, const float *knob,
                       int knob_stride, float *inp_next, void *stream);
int ra_weighted_sum_multi_f32(const float *w, const float *bias, const float *y, int B, int N, int T,
                              int HW, float *out, void *stream);
/* ... with out[b][n] written at b * o_img + n * o_row (floats, multiples of 4): the gradient of timestep-major masks. */
int ra_weighted_sum_multi_strided_f32(const float *w, const float *bias, const float *y, int B, int N, int T, int HW,
                                      float *out, size_t o_img, size_t o_row, void *stream);

/* Dynamic tile tickets for the persistent controller-CNN launches (no reference counterpart: nnlib.cnn, nnlib.py:229-253, is
 * one TF op per layer and knows no tiles).  ra_conv_pair_cached_f32, ra_conv_pair_wino_f32, ra_conv_wino_f32 and
 * ra_conv_split_f32 run persistent grids; by default a workgroup walks a fixed list of tiles, which is fastest when the
 * launch owns the GPU and up to 2x slower when other work (another batch's controller in the decode pipeline, another
 * process) keeps some of its workgroups from starting on time.  Between ra_tile_tickets_bind(scratch, slots) and
 * ra_tile_tickets_bind(NULL, 0) every such launch issued by the CALLING THREAD takes the next slot(s) of `scratch` (one per
 * output-channel slice) and its workgroups DRAW their tiles from per-XCD pools in it, so that a late workgroup costs only
 * its share.  scratch: device memory, 128-byte aligned, slots * ra_tile_tickets_slot_bytes() bytes, ZERO when the first of
 * those launches executes (e.g. ra_fill_f32 on the same stream), used by launches of ONE stream only, and re-zeroed before the
 * slots are handed out again (the decode engine binds at the start of a forward: one fill per forward, also inside its
 * captured graph).  Launches that find no slot left, or whose grid is too small to draw from all eight pools, keep the
 * static walk.  Returns 1 if bound, 0 if unbound (NULL, or a device whose workgroups do not report exactly the XCC ids
 * 0..7: the static walk stays), negative on error.  RA_TILE_TICKETS=0 disables it. */
int ra_tile_tickets_bind(void *scratch, int slots);
int ra_tile_tickets_slot_bytes(void);

/* p[0..n) = value (p 16-byte aligned): the canvas reset `canvas = zeros` (full_model.py:239) and
 * the sigmoid(beta) prefill of y_out behind RA_PASTE_Y_PREFILLED, as a library launch so that the
 * captured forward holds no framework kernel. */
int ra_fill_f32(float *p, size_t n, float value, void *stream);
/* out[i] = idx[i] >= 0 ? src[idx[i]] : 0 for i < n (device pointers).  The training step re-packs the controller's
 * weights for the decode loop's kernels once per optimisation step without leaving the device: the host packers
 * (ra_ctrl_split_pack_weights ...) only move values, so packing arrays of flat-bucket positions once gives the index map. */
int ra_gather_f32(const float *src, const int *idx, size_t n, float *out, void *stream);
/* C [M, N] += A^T B (and bias [N] += the column sums of B) over the rows k < K of the row-major A [K, M] (row stride lda)
 * and B [K, N] (ldb): the parameter gradients tf.gradients forms for the controller's dense layers (nnlib.mlp /
 * nnlib.lstm, full_model.py:668-689) from a step's layer inputs (A) and pre-activation gradients (B) of every
 * (timestep, image, glimpse iteration) — K is a few hundred rows, the output wide.  k_period > 0 skips the rows with
 * k % k_period == k_period - 1 (the last glimpse iteration of an image feeds no next one).  seg == NULL: plain C (row stride
 * ldc), bias or NULL.  seg != NULL: a DEVICE table of 3 * ceil(N / col_block) pointers, [rows < row_split | rows >=
 * row_split | bias] x column block (NULL entries skipped): every block is its own dense [rows, col_block] tensor — the
 * LSTM's eight weight and four bias parameters of the flat gradient bucket; row_split % 16 == col_block % 16 == 0. */
int ra_gemm_tn_acc_f32(const float *A, int lda, const float *B, int ldb, int K, int M, int N, int k_period, float *C, int ldc,
                       float *bias, const void *const *seg, int row_split, int col_block, void *stream);
/* modellib.f_greedy_match with matched == 0 (modellib.py:365-379; box_model.py:487-498):
 * match[b,t] = (score[b,t] == max_t score[b,:]) / #maxima.  score, match [B,T]. */
int ra_greedy_match_f32(const float *score, int B, int T, float *match, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* RECATTEND_H_ */
