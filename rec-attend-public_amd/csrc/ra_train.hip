// Training-step kernels (full_model.py:1039-1057 and the backward passes they need) that belong to no larger family: the Adam
// step, the device-side weight repack and the odd-pixel subsample of a conv layer's backward, the soft-IoU adjoint, the canvas
// step, the LSTM cell, the Gauss filter bank, the attention head and the knob mix.  The conv kernels are in ra_conv*.hip, the
// filter gradients in ra_wgrad.hip, train-mode BatchNorm in ra_bn.hip, the controller's training kernels in ra_ctrl_train.hip.
//
// ra_adam_step_f32 — the reference's optimizer on ONE flat float32 bucket:
//   gvs = optimizer.compute_gradients(total_loss); grad = clip_by_value(grad, -1, 1);
//   tf.train.AdamOptimizer(learn_rate, epsilon=1e-7).apply_gradients          full_model.py:1048-1056
// with the weight-decay term wd * l2_loss(w) of nnlib.weight_variable (nnlib.py:59-61), which is
// part of total_loss and therefore of the clipped gradient, and the data-parallel mean
// (grad_scale = 1 / world after the RCCL sum) folded in — one pass over five arrays, HBM-bound.
// TF's Adam: lr_t = lr * sqrt(1 - b2^t) / (1 - b1^t); m = b1 m + (1-b1) g; v = b2 v + (1-b2) g^2;
//            p -= lr_t * m / (sqrt(v) + eps)        (epsilon outside the bias correction).
#include "ra_common.h"

namespace ra {
namespace train {
typedef float f32x4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(256) void adam_kernel(float *p, const float *g, float *m, float *v, const float *wd,
                                                   size_t n, float lr_t, float b1, float b2, float eps, float clip,
                                                   float gscale, const int *status, int n_solver, int n_other) {
  // the guarded form: a NEGATIVE solver status of this step (a matching that hit one of the reference's LOG(FATAL) caps; 1 =
  // the outer cap, where the reference logs and carries on with the partial matching, hungarian.cc:363-377) or any NON-ZERO
  // other word (a controller workgroup that timed out, another rank's failure flag) and the update is NOT applied —
  // parameters and moments stay as they are.  The words are uniform across the grid (scalar loads), written by launches
  // earlier on the stream.
  for (int k = 0; k < n_solver; ++k)
    if (status[k] < 0) return;
  for (int k = 0; k < n_other; ++k)
    if (status[n_solver + k] != 0) return;
  const size_t stride = (size_t)gridDim.x * 256;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
    const float pi = p[i];
    float gi = g[i] * gscale + (wd ? wd[i] * pi : 0.f);
    gi = fminf(fmaxf(gi, -clip), clip);
    const float mi = b1 * m[i] + (1.f - b1) * gi;
    const float vi = b2 * v[i] + (1.f - b2) * gi * gi;
    m[i] = mi;
    v[i] = vi;
    p[i] = pi - lr_t * mi / (sqrtf(vi) + eps);
  }
}
}  // namespace train
}  // namespace ra

using namespace ra;

extern "C" int ra_adam_step_f32(float *params, const float *grads, float *m, float *v, const float *wd_coef,
                                size_t n, float lr_t, float beta1, float beta2, float eps, float clip,
                                float grad_scale, void *stream) {
  if (!params || !grads || !m || !v) return fail(RA_E_INVALID, "ra_adam_step_f32: null pointer");
  if (n == 0) return 0;
  size_t grid = (n + 255) / 256;
  if (grid > 2048) grid = 2048;
  hipLaunchKernelGGL(train::adam_kernel, dim3((unsigned)grid), dim3(256), 0, as_stream(stream), params, grads, m, v,
                     wd_coef, n, lr_t, beta1, beta2, eps, clip, grad_scale, (const int *)nullptr, 0, 0);
  return launch_status("ra_adam_step_f32");
}

extern "C" int ra_adam_step_guarded_f32(float *params, const float *grads, float *m, float *v, const float *wd_coef,
                                        size_t n, float lr_t, float beta1, float beta2, float eps, float clip,
                                        float grad_scale, const int *status, int n_solver, int n_other, void *stream) {
  if (!params || !grads || !m || !v) return fail(RA_E_INVALID, "ra_adam_step_guarded_f32: null pointer");
  if (n_solver < 0 || n_other < 0 || (n_solver + n_other > 0 && !status))
    return fail(RA_E_INVALID, "ra_adam_step_guarded_f32: status words");
  if (n == 0) return 0;
  size_t grid = (n + 255) / 256;
  if (grid > 2048) grid = 2048;
  hipLaunchKernelGGL(train::adam_kernel, dim3((unsigned)grid), dim3(256), 0, as_stream(stream), params, grads, m, v,
                     wd_coef, n, lr_t, beta1, beta2, eps, clip, grad_scale, status, n_solver, n_other);
  return launch_status("ra_adam_step_guarded_f32");
}

namespace ra {
namespace train {
// ---- device-side weight repack (the host form is ra_conv_pack_weights) ----
__global__ void pack_weights_kernel(const float *w, int Cin_w, int Cout, int Cin, const int *chan_map, int tr, int CK,
                                    int cp, float *out) {
  const int total = 9 * Cin * cp;
  const int NCG = CK / 4;
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
    const int co = e % cp;
    int r = e / cp;
    const int ksub = r % 4;
    r /= 4;
    const int cg = r % NCG;
    r /= NCG;
    const int tap = r % 9, chunk = r / 9;
    const int c = chunk * CK + cg * 4 + ksub;
    const int src_c = chan_map ? chan_map[c] : c;
    const int ky = tap / 3, kx = tap % 3;
    float v = 0.f;
    if (co < Cout && src_c >= 0) {
      if (!tr)
        v = w[(((size_t)ky * 3 + kx) * Cin_w + src_c) * Cout + co];
      else
        v = w[(((size_t)(2 - ky) * 3 + (2 - kx)) * Cout + co) * Cin_w + src_c];
    }
    out[e] = v;
  }
}

// ---- y[b,i,j,:] = x[b,2i+1,2j+1,:]: the adjoint of the zero-stuffing of a stride-2 transposed conv ----
__global__ __launch_bounds__(256) void subsample_odd_kernel(const float *x, int B, int H, int W, int C, float *y) {
  const size_t total = (size_t)B * H * W * C;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
    const int c = (int)(e % C);
    size_t r = e / C;
    const int j = (int)(r % W);
    r /= W;
    const int i = (int)(r % H), b = (int)(r / H);
    y[e] = x[(((size_t)b * 2 * H + 2 * i + 1) * 2 * W + 2 * j + 1) * C + c];
  }
}

// ---- out[b,n,p] = sum_t w[b,n,t] * y[b,t,p] + bias[b,n]: the adjoint of the pairwise soft IoU ----
__global__ __launch_bounds__(256) void weighted_sum_multi_kernel(const float *w, const float *bias, const float *y, int N,
                                                                 int T, int HW, float *out, size_t o_img, size_t o_row) {
  const int b = blockIdx.z, n = blockIdx.y;
  const int e = (blockIdx.x * 256 + threadIdx.x) * 4;
  if (e >= HW) return;
  const float *yb = y + (size_t)b * T * HW + e;
  const float b0 = bias ? bias[(size_t)b * N + n] : 0.f;
  f32x4 acc = f32x4{b0, b0, b0, b0};
  for (int t = 0; t < T; ++t) {
    const float wt = w[((size_t)b * N + n) * T + t];
    if (wt != 0.f) acc += wt * *reinterpret_cast<const f32x4 *>(yb + (size_t)t * HW);  // uniform per (b, n)
  }
  *reinterpret_cast<f32x4 *>(out + (size_t)b * o_img + (size_t)n * o_row + e) = acc;
}

// ---- the canvas of the next timestep (full_model.py:826-848), written straight into the next packed controller-CNN
// input: per pixel   g = sum_t match[b,t] y_gt[b,t,p];  g -= g * noise[b,p];  y_c = knob[b] g + (1 - knob[b]) y[b,p];
// canvas' = max(y_c, canvas)   (no knob: y_c = y), every product and sum rounded on its own like the element-wise
// chain it replaces.  nxt[b,p,:] = prev[b,p,:] with channel `cc` = canvas'.  C in {4, 8, ...}: one float4 group of the
// pixel holds the canvas; the other groups are copied. ----
__global__ __launch_bounds__(256) void canvas_step_kernel(const f32x4 *prev, int C4, int cc, int HW, const float *y,
                                                          const float *match, const float *y_gt, int T, const float *noise,
                                                          const float *knob, int knob_stride, f32x4 *nxt) {
  const int b = blockIdx.y, p = blockIdx.x * 256 + threadIdx.x;
  if (p >= HW) return;
  const size_t px = (size_t)b * HW + p;
  float yc = y[px];
  if (match) {
    float g = 0.f;
    const float *yb = y_gt + (size_t)b * T * HW + p;
    for (int t = 0; t < T; ++t) {
      const float wt = match[(size_t)b * T + t];
      if (wt != 0.f) g = add_rn(g, mul_rn(wt, yb[(size_t)t * HW]));  // uniform per image
    }
    if (noise) g = sub_rn(g, mul_rn(g, noise[px]));
    const float k = knob[(size_t)b * knob_stride];
    yc = add_rn(mul_rn(k, g), mul_rn(sub_rn(1.0f, k), yc));
  }
  const int cg = cc >> 2, cl = cc & 3;
  for (int q = 0; q < C4; ++q) {
    f32x4 v = prev[px * C4 + q];
    if (q == cg) v[cl] = fmaxf(yc, v[cl]);
    nxt[px * C4 + q] = v;
  }
}

}  // namespace train
}  // namespace ra

extern "C" int ra_canvas_step_f32(const float *inp_prev, int C, int canvas_chan, int B, int HW, const float *y, const float *match,
                                  const float *y_gt, int T, const float *noise, const float *knob, int knob_stride,
                                  float *inp_next, void *stream) {
  if (!inp_prev || !y || !inp_next || B <= 0 || HW <= 0 || C <= 0 || C % 4 || canvas_chan < 0 || canvas_chan >= C ||
      (match && (!y_gt || !knob || T <= 0 || knob_stride < 1)))
    return fail(RA_E_INVALID, "ra_canvas_step_f32: bad argument");
  hipLaunchKernelGGL(train::canvas_step_kernel, dim3(ceil_div(HW, 256), B), dim3(256), 0, as_stream(stream),
                     reinterpret_cast<const train::f32x4 *>(inp_prev), C / 4, canvas_chan, HW, y, match, y_gt, T, noise, knob,
                     knob_stride, reinterpret_cast<train::f32x4 *>(inp_next));
  return launch_status("ra_canvas_step_f32");
}

extern "C" int ra_conv_pack_weights_dev(const float *w, int Cin_w, int Cout, int Cin, const int *chan_map, int flags,
                                        float *out, void *stream) {
  const int cp = ra_conv_cout_padded(Cout);
  if (!w || !out || Cin_w <= 0 || Cin <= 0) return fail(RA_E_INVALID, "ra_conv_pack_weights_dev: bad argument");
  if (Cin % 4 || !cp) return fail(RA_E_SHAPE, "ra_conv_pack_weights_dev: Cin %d %% 4 or Cout %d", Cin, Cout);
  if (!chan_map && Cin_w != Cin) return fail(RA_E_SHAPE, "ra_conv_pack_weights_dev: Cin_w != Cin without map");
  const int CK = (Cin % 16 == 0) ? 16 : (Cin % 8 == 0) ? 8 : 4;
  const int total = 9 * Cin * cp;
  hipLaunchKernelGGL(train::pack_weights_kernel, dim3(ceil_div(total, 256)), dim3(256), 0, as_stream(stream), w, Cin_w, Cout,
                     Cin, chan_map, (flags & RA_CONV_TRANSPOSED) ? 1 : 0, CK, cp, out);
  return launch_status("ra_conv_pack_weights_dev");
}

extern "C" int ra_subsample_odd_f32(const float *x, int B, int H, int W, int C, float *y, void *stream) {
  if (!x || !y || B <= 0 || H <= 0 || W <= 0 || C <= 0) return fail(RA_E_INVALID, "ra_subsample_odd_f32: bad argument");
  size_t grid = ((size_t)B * H * W * C + 255) / 256;
  if (grid > 8192) grid = 8192;
  hipLaunchKernelGGL(train::subsample_odd_kernel, dim3((unsigned)grid), dim3(256), 0, as_stream(stream), x, B, H, W, C, y);
  return launch_status("ra_subsample_odd_f32");
}

extern "C" int ra_weighted_sum_multi_strided_f32(const float *w, const float *bias, const float *y, int B, int N, int T, int HW,
                                                 float *out, size_t o_img, size_t o_row, void *stream);
extern "C" int ra_weighted_sum_multi_f32(const float *w, const float *bias, const float *y, int B, int N, int T, int HW,
                                         float *out, void *stream) {
  return ra_weighted_sum_multi_strided_f32(w, bias, y, B, N, T, HW, out, (size_t)N * HW, (size_t)HW, stream);
}
// out[b][n] at b * o_img + n * o_row (floats): the gradient of timestep-major masks is written timestep-major
extern "C" int ra_weighted_sum_multi_strided_f32(const float *w, const float *bias, const float *y, int B, int N, int T, int HW,
                                                 float *out, size_t o_img, size_t o_row, void *stream) {
  if ((o_img | o_row) & 3) return fail(RA_E_SHAPE, "ra_weighted_sum_multi_strided_f32: strides must be multiples of 4 floats");
  if (!w || !y || !out || B <= 0 || N <= 0 || T <= 0 || HW <= 0)
    return fail(RA_E_INVALID, "ra_weighted_sum_multi_f32: bad argument");
  if (HW % 4 || ((reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(out)) & 15))
    return fail(RA_E_SHAPE, "ra_weighted_sum_multi_f32: H*W %% 4 and 16-byte aligned tensors required");
  hipLaunchKernelGGL(train::weighted_sum_multi_kernel, dim3(ceil_div(HW, 1024), N, B), dim3(256), 0, as_stream(stream), w,
                     bias, y, N, T, HW, out, o_img, o_row);
  return launch_status("ra_weighted_sum_multi_f32");
}

namespace ra {
namespace train {
// ---- LSTM cell pointwise part (nnlib.py:641-646): pre [B][4*hid] = the four gate pre-activations
// (i, f, o, u), c_prev [B][hid]  ->  c = f c_prev + i u,  h = o tanh(c).  act keeps the gate values
// for the backward; one thread per (image, unit).
__global__ __launch_bounds__(256) void lstm_cell_kernel(const float *pre, const float *c_prev, int n, int hid, float *h,
                                                        float *c, float *act) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= n) return;
  const int b = idx / hid, j = idx - b * hid;
  const float *p = pre + (size_t)b * 4 * hid + j;
  const float gi = 1.f / (1.f + expf(-p[0])), gf = 1.f / (1.f + expf(-p[hid])), go = 1.f / (1.f + expf(-p[2 * hid])),
              gu = tanhf(p[3 * hid]);
  const float cn = gf * c_prev[idx] + gi * gu;
  float *a = act + (size_t)b * 4 * hid + j;
  a[0] = gi;
  a[hid] = gf;
  a[2 * hid] = go;
  a[3 * hid] = gu;
  c[idx] = cn;
  h[idx] = go * tanhf(cn);
}
__global__ __launch_bounds__(256) void lstm_cell_bwd_kernel(const float *act, const float *c_prev, const float *c,
                                                            const float *dh, const float *dc, int n, int hid, float *dpre,
                                                            float *dc_prev) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= n) return;
  const int b = idx / hid, j = idx - b * hid;
  const float *a = act + (size_t)b * 4 * hid + j;
  const float gi = a[0], gf = a[hid], go = a[2 * hid], gu = a[3 * hid];
  const float tc = tanhf(c[idx]);
  const float gh = dh ? dh[idx] : 0.f;
  const float dcn = (dc ? dc[idx] : 0.f) + gh * go * (1.f - tc * tc);
  float *d = dpre + (size_t)b * 4 * hid + j;
  d[0] = dcn * gu * gi * (1.f - gi);
  d[hid] = dcn * c_prev[idx] * gf * (1.f - gf);
  d[2 * hid] = gh * tc * go * (1.f - go);
  d[3 * hid] = dcn * gi * (1.f - gu * gu);
  dc_prev[idx] = dcn * gf;
}

// ---- Gaussian filter bank (modellib.py:581-612): F[b][l][j] = N(l; mu_j, var), mu_j = ctr + (size + 1) / NF * (j - (NF - 1) / 2),
// var = exp(lg_var); its adjoint reduces over the whole [L, NF] bank of an image: one workgroup per image.
// sc / ss / sv: elements between consecutive images in ctr / size / lg_var (1: a dense [B] vector; the training graph
// hands in one column of a [B,2] tensor without copying it out)
__global__ __launch_bounds__(256) void gauss_filter_kernel(const float *ctr, const float *size, const float *lg_var, int sc,
                                                           int ss, int sv, int L, int NF, float *out) {
  const int b = blockIdx.y, e = blockIdx.x * 256 + threadIdx.x;
  if (e >= L * NF) return;
  const int l = e / NF, j = e - l * NF;
  const float var = expf(lg_var[(size_t)b * sv]);
  const float mu = ctr[(size_t)b * sc] + (size[(size_t)b * ss] + 1.0f) / (float)NF * ((float)j - 0.5f * (float)(NF - 1));
  const float dd = (float)l - mu;
  out[(size_t)b * L * NF + e] = expf(-0.5f * dd * dd / var) / (sqrtf(var) * 2.5066282746310002f);
}
__global__ __launch_bounds__(256) void gauss_filter_bwd_kernel(const float *ctr, const float *size, const float *lg_var,
                                                               int sc, int ss, int sv, const float *g, int L, int NF,
                                                               float *dctr, float *dsize, float *dlgv, int sd) {
  __shared__ float red[256];
  const int b = blockIdx.x;
  const float var = expf(lg_var[(size_t)b * sv]), c0 = ctr[(size_t)b * sc], step = (size[(size_t)b * ss] + 1.0f) / (float)NF;
  const float norm = 1.0f / (sqrtf(var) * 2.5066282746310002f);
  float a_ctr = 0.f, a_size = 0.f, a_var = 0.f;
  for (int e = threadIdx.x; e < L * NF; e += 256) {
    const int l = e / NF, j = e - l * NF;
    const float off = (float)j - 0.5f * (float)(NF - 1);
    const float dd = (float)l - (c0 + step * off);
    const float f = expf(-0.5f * dd * dd / var) * norm;
    const float gf = g[(size_t)b * L * NF + e] * f;
    const float dmu = gf * dd / var;
    a_ctr += dmu;
    a_size += dmu * off / (float)NF;
    a_var += gf * (0.5f * dd * dd / (var * var) - 0.5f / var);
  }
  a_ctr = block_sum256(a_ctr, red);
  a_size = block_sum256(a_size, red);
  a_var = block_sum256(a_var, red);
  if (threadIdx.x == 0) {
    dctr[(size_t)b * sd] = a_ctr;
    dsize[(size_t)b * sd] = a_size;
    dlgv[(size_t)b * sd] = a_var * var;
  }
}

}  // namespace train
}  // namespace ra

extern "C" int ra_lstm_cell_f32(const float *pre, const float *c_prev, int B, int hid, float *h, float *c, float *act,
                                void *stream) {
  if (!pre || !c_prev || !h || !c || !act || B <= 0 || hid <= 0) return fail(RA_E_INVALID, "ra_lstm_cell_f32: bad argument");
  const int n = B * hid;
  hipLaunchKernelGGL(train::lstm_cell_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, as_stream(stream), pre, c_prev, n, hid, h, c,
                     act);
  return launch_status("ra_lstm_cell_f32");
}

extern "C" int ra_lstm_cell_bwd_f32(const float *act, const float *c_prev, const float *c, const float *dh, const float *dc,
                                    int B, int hid, float *dpre, float *dc_prev, void *stream) {
  if (!act || !c_prev || !c || !dpre || !dc_prev || B <= 0 || hid <= 0)
    return fail(RA_E_INVALID, "ra_lstm_cell_bwd_f32: bad argument");
  const int n = B * hid;
  hipLaunchKernelGGL(train::lstm_cell_bwd_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, as_stream(stream), act, c_prev, c, dh,
                     dc, n, hid, dpre, dc_prev);
  return launch_status("ra_lstm_cell_bwd_f32");
}

extern "C" int ra_gauss_filter_strided_f32(const float *ctr, const float *size, const float *lg_var, int stride_ctr,
                                           int stride_size, int stride_lg_var, int B, int L, int NF, float *out, void *stream) {
  if (!ctr || !size || !lg_var || !out || B <= 0 || L <= 0 || NF <= 0 || stride_ctr < 1 || stride_size < 1 || stride_lg_var < 0)
    return fail(RA_E_INVALID, "ra_gauss_filter_f32: bad argument");
  hipLaunchKernelGGL(train::gauss_filter_kernel, dim3(ceil_div(L * NF, 256), B), dim3(256), 0, as_stream(stream), ctr, size,
                     lg_var, stride_ctr, stride_size, stride_lg_var, L, NF, out);
  return launch_status("ra_gauss_filter_f32");
}
extern "C" int ra_gauss_filter_f32(const float *ctr, const float *size, const float *lg_var, int B, int L, int NF, float *out,
                                   void *stream) {
  return ra_gauss_filter_strided_f32(ctr, size, lg_var, 1, 1, 1, B, L, NF, out, stream);
}

extern "C" int ra_gauss_filter_strided_bwd_f32(const float *ctr, const float *size, const float *lg_var, int stride_ctr,
                                               int stride_size, int stride_lg_var, const float *g, int B, int L, int NF,
                                               float *dctr, float *dsize, float *dlg_var, int stride_grad, void *stream) {
  if (!ctr || !size || !lg_var || !g || !dctr || !dsize || !dlg_var || B <= 0 || L <= 0 || NF <= 0 || stride_ctr < 1 ||
      stride_size < 1 || stride_lg_var < 0 || stride_grad < 1)
    return fail(RA_E_INVALID, "ra_gauss_filter_bwd_f32: bad argument");
  hipLaunchKernelGGL(train::gauss_filter_bwd_kernel, dim3(B), dim3(256), 0, as_stream(stream), ctr, size, lg_var, stride_ctr,
                     stride_size, stride_lg_var, g, L, NF, dctr, dsize, dlg_var, stride_grad);
  return launch_status("ra_gauss_filter_bwd_f32");
}
extern "C" int ra_gauss_filter_bwd_f32(const float *ctr, const float *size, const float *lg_var, const float *g, int B, int L,
                                       int NF, float *dctr, float *dsize, float *dlg_var, void *stream) {
  return ra_gauss_filter_strided_bwd_f32(ctr, size, lg_var, 1, 1, 1, g, B, L, NF, dctr, dsize, dlg_var, 1, stream);
}

// ---- the attention head of the training graph: controller output -> attention parameters (full_model.py:702-722,
// modellib.py:752-764,812-825), and the ground-truth knob on them (full_model.py:744-773).  Scalar math on nine numbers
// per image; as separate torch ops it was ~45 launches per timestep forward + backward. ----
namespace ra {
namespace train {
constexpr int kHeadStride = 16;  // floats per image in the head's output record
// record: [0,1] cn  [2,3] ls  [4,5] ctr  [6,7] size  [8,9] lg_var  [10] attn_gamma  [11] box_gamma  [12] y_lg_gamma
__device__ inline float softplus_t(float x) { return x > 20.f ? x : log1pf(expf(x)); }  // torch.nn.functional.softplus
__global__ __launch_bounds__(64) void attn_head_kernel(const float *co, int sco, int B, float H, float W, float Fh, float Fw,
                                                       int flags, float *out, float *arec) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  const float *c = co + (size_t)b * sco;
  float *o = out + (size_t)b * kHeadStride;
  const bool squash = flags & 1, fixed_var = flags & 2, dynamic_var = flags & 4, fixed_gamma = flags & 8;
  const float dim[2] = {H, W}, fs[2] = {Fh, Fw};
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const float cn = squash ? tanhf(c[k]) : c[k];
    const float ls = squash ? -softplus_t(c[2 + k]) : c[2 + k];
    const float ctr = (cn + 1.0f) * dim[k] / 2.0f, size = expf(ls) * dim[k];
    float lv = fixed_var ? 0.f : logf(size) - logf(fs[k]);
    if (dynamic_var) lv = c[4 + k];
    o[k] = cn;
    o[2 + k] = ls;
    o[4 + k] = ctr;
    o[6 + k] = size;
    o[8 + k] = lv;
  }
  o[10] = fixed_gamma ? 1.f : expf(c[6]);
  o[11] = expf(c[7]);
  o[12] = fixed_gamma ? 2.f : c[8];
  if (arec) {  // the same window as the resample kernels' attention record (ctr, size, lg_var, the three gammas, zeros)
    float *r = arec + (size_t)b * RA_ATTN_STRIDE;
#pragma unroll
    for (int k = 0; k < 2; ++k) r[k] = o[4 + k], r[2 + k] = o[6 + k], r[4 + k] = o[8 + k];
    r[6] = o[10], r[7] = o[11], r[8] = o[12];
#pragma unroll
    for (int k = 9; k < RA_ATTN_STRIDE; ++k) r[k] = 0.f;
  }
}
// g_*: gradients of the record's fields, each nullable (no gradient = zero), dense [B,2] / [B]
__global__ __launch_bounds__(64) void attn_head_bwd_kernel(const float *co, int sco, const float *out, const float *g_cn,
                                                           const float *g_ls, const float *g_ctr, const float *g_size,
                                                           const float *g_lv, const float *g_ag, const float *g_bg,
                                                           const float *g_ylg, int B, float H, float W, int flags, float *dco) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  const float *c = co + (size_t)b * sco, *o = out + (size_t)b * kHeadStride;
  float *d = dco + (size_t)b * 9;
  const bool squash = flags & 1, fixed_var = flags & 2, dynamic_var = flags & 4, fixed_gamma = flags & 8;
  const float dim[2] = {H, W};
  auto at2 = [&](const float *g, int k) { return g ? g[2 * b + k] : 0.f; };
  auto at1 = [&](const float *g) { return g ? g[b] : 0.f; };
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const float cn = o[k], size = o[6 + k];
    const float d_cn = at2(g_cn, k) + at2(g_ctr, k) * dim[k] / 2.0f;
    // size = exp(ls) dim, lg_var = ls + log(dim / F): both follow ls
    const float d_ls = at2(g_ls, k) + at2(g_size, k) * size + ((fixed_var || dynamic_var) ? 0.f : at2(g_lv, k));
    d[k] = squash ? d_cn * (1.0f - cn * cn) : d_cn;
    const float x = c[2 + k];
    d[2 + k] = squash ? d_ls * (x > 20.f ? -1.0f : -1.0f / (1.0f + expf(-x))) : d_ls;
    d[4 + k] = dynamic_var ? at2(g_lv, k) : 0.f;
  }
  d[6] = fixed_gamma ? 0.f : at1(g_ag) * o[10];
  d[7] = at1(g_bg) * o[11];
  d[8] = fixed_gamma ? 0.f : at1(g_ylg);
}
// p2 = kb m + (1 - kb) p for the window centre and size, m = sum_t match[b][t] gt[b][t][:] (the matched noisy GT box)
__global__ __launch_bounds__(64) void knob_mix_kernel(const float *ctr, const float *size, const float *match, const float *ctr_gt,
                                                      const float *size_gt, const float *kb, int skb, int sp, int B, int T,
                                                      float *ctr2, float *size2, const float *arec, float *arec2) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  float mc[2] = {0.f, 0.f}, ms[2] = {0.f, 0.f};
  for (int t = 0; t < T; ++t) {
    const float w = match[(size_t)b * T + t];
    mc[0] += w * ctr_gt[((size_t)b * T + t) * 2];
    mc[1] += w * ctr_gt[((size_t)b * T + t) * 2 + 1];
    ms[0] += w * size_gt[((size_t)b * T + t) * 2];
    ms[1] += w * size_gt[((size_t)b * T + t) * 2 + 1];
  }
  const float k = kb[(size_t)b * skb];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    ctr2[2 * b + i] = k * mc[i] + (1.0f - k) * ctr[(size_t)b * sp + i];
    size2[2 * b + i] = k * ms[i] + (1.0f - k) * size[(size_t)b * sp + i];
  }
  if (arec2) {  // the attention record with the mixed window (variance and gammas as predicted)
    const float *r = arec + (size_t)b * RA_ATTN_STRIDE;
    float *r2 = arec2 + (size_t)b * RA_ATTN_STRIDE;
#pragma unroll
    for (int i = 0; i < 2; ++i) r2[i] = ctr2[2 * b + i], r2[2 + i] = size2[2 * b + i];
#pragma unroll
    for (int i = 4; i < RA_ATTN_STRIDE; ++i) r2[i] = r[i];
  }
}
__global__ __launch_bounds__(64) void knob_mix_bwd_kernel(const float *g_ctr2, const float *g_size2, const float *kb, int skb, int B,
                                                          float *d_ctr, float *d_size) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  const float k = 1.0f - kb[(size_t)b * skb];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    d_ctr[2 * b + i] = g_ctr2 ? k * g_ctr2[2 * b + i] : 0.f;
    d_size[2 * b + i] = g_size2 ? k * g_size2[2 * b + i] : 0.f;
  }
}
}  // namespace train
}  // namespace ra

extern "C" int ra_attn_head_rec_f32(const float *ctrl_out, int stride, int B, int H, int W, int Fh, int Fw, int flags, float *out,
                                    float *attn_rec, void *stream) {
  if (!ctrl_out || !out || B <= 0 || stride < 9) return fail(RA_E_INVALID, "ra_attn_head_f32: bad argument");
  hipLaunchKernelGGL(train::attn_head_kernel, dim3(ceil_div(B, 64)), dim3(64), 0, as_stream(stream), ctrl_out, stride, B, (float)H,
                     (float)W, (float)Fh, (float)Fw, flags, out, attn_rec);
  return launch_status("ra_attn_head_f32");
}
extern "C" int ra_attn_head_f32(const float *ctrl_out, int stride, int B, int H, int W, int Fh, int Fw, int flags, float *out,
                                void *stream) {
  return ra_attn_head_rec_f32(ctrl_out, stride, B, H, W, Fh, Fw, flags, out, nullptr, stream);
}
extern "C" int ra_attn_head_bwd_f32(const float *ctrl_out, int stride, const float *out, const float *g_cn, const float *g_ls,
                                    const float *g_ctr, const float *g_size, const float *g_lg_var, const float *g_attn_gamma,
                                    const float *g_box_gamma, const float *g_y_lg_gamma, int B, int H, int W, int flags,
                                    float *d_ctrl_out, void *stream) {
  if (!ctrl_out || !out || !d_ctrl_out || B <= 0 || stride < 9) return fail(RA_E_INVALID, "ra_attn_head_bwd_f32: bad argument");
  hipLaunchKernelGGL(train::attn_head_bwd_kernel, dim3(ceil_div(B, 64)), dim3(64), 0, as_stream(stream), ctrl_out, stride, out, g_cn,
                     g_ls, g_ctr, g_size, g_lg_var, g_attn_gamma, g_box_gamma, g_y_lg_gamma, B, (float)H, (float)W, flags,
                     d_ctrl_out);
  return launch_status("ra_attn_head_bwd_f32");
}
extern "C" int ra_knob_mix_rec_f32(const float *ctr, const float *size, const float *match, const float *ctr_gt, const float *size_gt,
                                   const float *knob, int knob_stride, int row_stride, int B, int T, float *ctr2, float *size2,
                                   const float *attn_rec, float *attn_rec2, void *stream) {
  if (!ctr || !size || !match || !ctr_gt || !size_gt || !knob || !ctr2 || !size2 || B <= 0 || T <= 0 || row_stride < 2 ||
      (attn_rec2 && !attn_rec))
    return fail(RA_E_INVALID, "ra_knob_mix_f32: bad argument");
  hipLaunchKernelGGL(train::knob_mix_kernel, dim3(ceil_div(B, 64)), dim3(64), 0, as_stream(stream), ctr, size, match, ctr_gt, size_gt,
                     knob, knob_stride, row_stride, B, T, ctr2, size2, attn_rec, attn_rec2);
  return launch_status("ra_knob_mix_f32");
}
extern "C" int ra_knob_mix_f32(const float *ctr, const float *size, const float *match, const float *ctr_gt, const float *size_gt,
                               const float *knob, int knob_stride, int row_stride, int B, int T, float *ctr2, float *size2,
                               void *stream) {
  return ra_knob_mix_rec_f32(ctr, size, match, ctr_gt, size_gt, knob, knob_stride, row_stride, B, T, ctr2, size2, nullptr, nullptr, stream);
}
extern "C" int ra_knob_mix_bwd_f32(const float *g_ctr2, const float *g_size2, const float *knob, int knob_stride, int B,
                                   float *d_ctr, float *d_size, void *stream) {
  if (!knob || !d_ctr || !d_size || B <= 0) return fail(RA_E_INVALID, "ra_knob_mix_bwd_f32: bad argument");
  hipLaunchKernelGGL(train::knob_mix_bwd_kernel, dim3(ceil_div(B, 64)), dim3(64), 0, as_stream(stream), g_ctr2, g_size2, knob,
                     knob_stride, B, d_ctr, d_size);
  return launch_status("ra_knob_mix_bwd_f32");
}
