// Training-step kernels (full_model.py:1039-1057 and the backward passes they need).
//
// ra_adam_step_f32 — the reference's optimizer on ONE flat float32 bucket:
//   gvs = optimizer.compute_gradients(total_loss); grad = clip_by_value(grad, -1, 1);
//   tf.train.AdamOptimizer(learn_rate, epsilon=1e-7).apply_gradients          full_model.py:1048-1056
// with the weight-decay term wd * l2_loss(w) of nnlib.weight_variable (nnlib.py:59-61), which is
// part of total_loss and therefore of the clipped gradient, and the data-parallel mean
// (grad_scale = 1 / world after the RCCL sum) folded in — one pass over five arrays, HBM-bound.
// TF's Adam: lr_t = lr * sqrt(1 - b2^t) / (1 - b1^t); m = b1 m + (1-b1) g; v = b2 v + (1-b2) g^2;
//            p -= lr_t * m / (sqrt(v) + eps)        (epsilon outside the bias correction).
#include <type_traits>

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
// =================================================================================================
// Fast forms of the BatchNorm elementwise / reduction passes for C % 4 == 0 with C / 4 a power of two
// (every layer of the three CNNs except 1- or 3-channel ends): a thread owns FOUR channels of one
// pooling window — float4 loads, 32-bit indices, the window's (up to 4) pixels read once instead of
// once per pixel, the per-channel constants hoisted (the grid stride is a multiple of C / 4, so a
// thread's channel group never changes).  The generic kernels above moved 0.5 TB/s.
// Summation order is fixed (no atomics): bit-reproducible.
struct BnConst {
  f32x4 mu, g, be, rstd;
};
// Storage of a channel quad: float32 (16 bytes) or, in the bf16 mode's tensors between the conv layers' passes
// (model_opt['compute_dtype'] = 'bf16'), bf16 (8 bytes; loads are exact, stores round to nearest even as v_cvt_pk_bf16_f32).
typedef unsigned u32x2q __attribute__((ext_vector_type(2)));
template <bool BF>
struct Q4 {
  typedef f32x4 T;
  static __device__ inline f32x4 ld(const T *p, size_t i) { return p[i]; }
  static __device__ inline void st(T *p, size_t i, const f32x4 v) { p[i] = v; }
};
template <>
struct Q4<true> {
  typedef u32x2q T;
  static __device__ inline f32x4 ld(const T *p, size_t i) {
    const u32x2q q = p[i];
    return f32x4{__builtin_bit_cast(float, q.x << 16), __builtin_bit_cast(float, q.x & 0xffff0000u),
                 __builtin_bit_cast(float, q.y << 16), __builtin_bit_cast(float, q.y & 0xffff0000u)};
  }
  static __device__ inline void st(T *p, size_t i, const f32x4 v) {
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
    p[i] = u32x2q{__builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{v.x, v.y}, bf16x2)),
                  __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{v.z, v.w}, bf16x2))};
  }
};
__device__ inline BnConst bn_const(const float *mean, const float *var, const float *gamma, const float *beta, float eps,
                                   int c0) {
  BnConst k;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float rstd = var ? rsqrtf(var[c0 + i] + eps) : 1.f;
    k.rstd[i] = rstd;
    k.g[i] = (gamma ? gamma[c0 + i] : 1.f) * rstd;
    k.mu[i] = mean ? mean[c0 + i] : 0.f;
    k.be[i] = beta ? beta[c0 + i] : 0.f;
  }
  return k;
}
// sum over the threads of a workgroup that share (tid % C4); valid in threads tid < C4.  C4 = 1 << lg <= 64.
__device__ inline float sum_by_group(float v, int C4, float *red) {
  for (int off = 32; off >= C4; off >>= 1) v += __shfl_xor(v, off, 64);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane < C4) red[wave * 64 + lane] = v;
  __syncthreads();
  float t = 0.f;
  if (threadIdx.x < C4) t = (red[threadIdx.x] + red[64 + threadIdx.x]) + (red[128 + threadIdx.x] + red[192 + threadIdx.x]);
  return t;
}

// per-channel sum (mean == nullptr) or sum of squared deviations over u [n4 = npix * C4] float4s
__global__ __launch_bounds__(256) void chan_sum_v4_kernel(const f32x4 *u, int n4, int C4, const float *mean, float *part) {
  __shared__ float red[256];
  const int tid = threadIdx.x, cg = tid & (C4 - 1);
  f32x4 mu = f32x4{0.f, 0.f, 0.f, 0.f};
  if (mean)
    for (int i = 0; i < 4; ++i) mu[i] = mean[4 * cg + i];
  f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int e = blockIdx.x * 256 + tid; e < n4; e += gridDim.x * 256) {
    const f32x4 v = u[e] - mu;
    s += mean ? v * v : v;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float t = sum_by_group(s[i], C4, red);
    if (tid < C4) part[(size_t)blockIdx.x * 4 * C4 + 4 * tid + i] = t;
  }
}

// the window of one thread: POOL x POOL pixels x 4 channels
template <int POOL, bool UB = false>
__device__ inline void load_window(const typename Q4<UB>::T *u, int b, int yo, int xo, int H, int W, int C4, int cg,
                                   f32x4 (&w)[POOL * POOL]) {
#pragma unroll
  for (int k = 0; k < POOL * POOL; ++k)
    w[k] = Q4<UB>::ld(u, ((b * H + yo * POOL + (k / POOL)) * W + xo * POOL + (k % POOL)) * C4 + cg);
}

template <int POOL>
constexpr int kRowsPerIter = POOL == 1 ? 4 : 1;  // output rows a thread of the float4 BatchNorm kernels handles per loop iteration

template <int POOL, bool UB = false, bool YB = false>
__global__ __launch_bounds__(256) void bn_act_pool_v4_kernel(const typename Q4<UB>::T *u, const float *mean, const float *var,
                                                             const float *gamma, const float *beta, float eps, int relu,
                                                             int B, int H, int W, int C4, int lg, typename Q4<YB>::T *y) {
  const int Ho = H / POOL, Wo = W / POOL;
  const int er = blockIdx.x * 256 + threadIdx.x;
  if (er >= Wo * C4) return;
  const int xo = er >> lg, cg = er & (C4 - 1);
  const BnConst k = bn_const(mean, var, gamma, beta, eps, 4 * cg);
  const float lo = relu ? 0.f : -__builtin_inff();
  // kRowsPerIter<POOL> rows per iteration, every load issued before the first use: a thread of the unpooled form moved 16
  // bytes per round trip (3.5 TB/s on the full-resolution layers; the pooled form's four loads per thread ran at 5.7)
  constexpr int RU = kRowsPerIter<POOL>;
  const int rows = B * Ho;
  for (int row0 = blockIdx.y * RU; row0 < rows; row0 += gridDim.y * RU) {
    f32x4 w[RU][POOL * POOL];
#pragma unroll
    for (int r = 0; r < RU; ++r)
      if (row0 + r < rows) {
        const int b = (row0 + r) / Ho, yo = (row0 + r) - b * Ho;
        load_window<POOL, UB>(u, b, yo, xo, H, W, C4, cg, w[r]);
      }
#pragma unroll
    for (int r = 0; r < RU; ++r)
      if (row0 + r < rows) {
        f32x4 best;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          float m = -__builtin_inff();
#pragma unroll
          for (int q = 0; q < POOL * POOL; ++q) m = fmaxf(m, fmaxf((w[r][q][i] - k.mu[i]) * k.g[i] + k.be[i], lo));
          best[i] = m;
        }
        Q4<YB>::st(y, ((row0 + r) * Wo + xo) * C4 + cg, best);
      }
  }
}

// dv of every pixel of the window (dy routed to the FIRST maximum, masked by the ReLU) and xhat
template <int POOL>
__device__ inline void window_grad(const f32x4 (&w)[POOL * POOL], const f32x4 dyv, const BnConst &k, float lo, int relu,
                                   f32x4 (&dv)[POOL * POOL], f32x4 (&xh)[POOL * POOL]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float best = -__builtin_inff();
    int arg = 0;
    float v[POOL * POOL];
#pragma unroll
    for (int q = 0; q < POOL * POOL; ++q) {
      xh[q][i] = (w[q][i] - k.mu[i]) * k.rstd[i];
      v[q] = (w[q][i] - k.mu[i]) * k.g[i] + k.be[i];
      const float a = fmaxf(v[q], lo);
      if (a > best) {
        best = a;
        arg = q;
      }
    }
#pragma unroll
    for (int q = 0; q < POOL * POOL; ++q) dv[q][i] = (q == arg && !(relu && v[q] <= 0.f)) ? dyv[i] : 0.f;
  }
}

template <int POOL, bool UB = false, bool DB = false>
__global__ __launch_bounds__(256) void bn_bwd_reduce_v4_kernel(const typename Q4<UB>::T *u, const typename Q4<DB>::T *dy, const float *mean,
                                                               const float *var, const float *gamma, const float *beta,
                                                               float eps, int relu, int B, int H, int W, int C4, int lg,
                                                               float *part, const float *const *tabs = nullptr, int G = 1) {
  __shared__ float red[256];
  const int Ho = H / POOL, Wo = W / POOL;
  if (tabs) {  // group blockIdx.z of G calls of the layer stacked along the batch: its own statistics and parameters
    const int g = blockIdx.z;
    mean = tabs[g], var = tabs[G + g], gamma = tabs[2 * G + g], beta = tabs[3 * G + g];
    u += (size_t)g * B * H * W * C4;
    dy += (size_t)g * B * Ho * Wo * C4;
    part += (size_t)g * gridDim.x * gridDim.y * 2 * 4 * C4;
  }
  const int er = blockIdx.x * 256 + threadIdx.x, tid = threadIdx.x;
  const bool live = er < Wo * C4;
  const int xo = er >> lg, cg = er & (C4 - 1);
  f32x4 s0 = f32x4{0.f, 0.f, 0.f, 0.f}, s1 = s0;
  if (live) {
    const BnConst k = bn_const(mean, var, gamma, beta, eps, 4 * cg);
    const float lo = relu ? 0.f : -__builtin_inff();
    for (int row = blockIdx.y; row < B * Ho; row += gridDim.y) {
      const int b = row / Ho, yo = row - b * Ho;
      f32x4 w[POOL * POOL], dv[POOL * POOL], xh[POOL * POOL];
      load_window<POOL, UB>(u, b, yo, xo, H, W, C4, cg, w);
      window_grad<POOL>(w, Q4<DB>::ld(dy, (row * Wo + xo) * C4 + cg), k, lo, relu, dv, xh);
#pragma unroll
      for (int q = 0; q < POOL * POOL; ++q) {
        s0 += dv[q];
        s1 += dv[q] * xh[q];
      }
    }
  }
  const int blk = blockIdx.y * gridDim.x + blockIdx.x, C = 4 * C4;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float t0 = sum_by_group(s0[i], C4, red), t1 = sum_by_group(s1[i], C4, red);
    if (tid < C4) {
      part[((size_t)blk * 2) * C + 4 * tid + i] = t0;
      part[((size_t)blk * 2 + 1) * C + 4 * tid + i] = t1;
    }
  }
}

template <int POOL, bool UB = false, bool DB = false>
__global__ __launch_bounds__(256) void bn_bwd_dx_v4_kernel(const typename Q4<UB>::T *u, const typename Q4<DB>::T *dy, const float *mean,
                                                           const float *var, const float *gamma, const float *beta,
                                                           const float *dbeta, const float *dgamma, float eps, int relu,
                                                           int B, int H, int W, int C4, int lg, typename Q4<UB>::T *du, float inv_n,
                                                           const float *const *tabs = nullptr, int G = 1) {
  const int Ho = H / POOL, Wo = W / POOL;
  if (tabs) {
    const int g = blockIdx.z;
    mean = tabs[g], var = tabs[G + g], gamma = tabs[2 * G + g], beta = tabs[3 * G + g];
    u += (size_t)g * B * H * W * C4;
    dy += (size_t)g * B * Ho * Wo * C4;
    du += (size_t)g * B * H * W * C4;
    dbeta += (size_t)g * 4 * C4;
    dgamma += (size_t)g * 4 * C4;
  }
  const int er = blockIdx.x * 256 + threadIdx.x;
  if (er >= Wo * C4) return;
  const int xo = er >> lg, cg = er & (C4 - 1);
  const BnConst k = bn_const(mean, var, gamma, beta, eps, 4 * cg);
  const float lo = relu ? 0.f : -__builtin_inff();
  f32x4 db, dg;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    db[i] = dbeta[4 * cg + i] * inv_n;
    dg[i] = dgamma[4 * cg + i] * inv_n;
  }
  constexpr int RU = kRowsPerIter<POOL>;
  const int rows = B * Ho;
  for (int row0 = blockIdx.y * RU; row0 < rows; row0 += gridDim.y * RU) {
    f32x4 w[RU][POOL * POOL], dyv[RU];
#pragma unroll
    for (int r = 0; r < RU; ++r)
      if (row0 + r < rows) {
        const int b = (row0 + r) / Ho, yo = (row0 + r) - b * Ho;
        load_window<POOL, UB>(u, b, yo, xo, H, W, C4, cg, w[r]);
        dyv[r] = Q4<DB>::ld(dy, ((row0 + r) * Wo + xo) * C4 + cg);
      }
#pragma unroll
    for (int r = 0; r < RU; ++r)
      if (row0 + r < rows) {
        const int b = (row0 + r) / Ho, yo = (row0 + r) - b * Ho;
        f32x4 dv[POOL * POOL], xh[POOL * POOL];
        window_grad<POOL>(w[r], dyv[r], k, lo, relu, dv, xh);
#pragma unroll
        for (int q = 0; q < POOL * POOL; ++q) {
          const f32x4 rr = var ? k.g * (dv[q] - db - xh[q] * dg) : dv[q];
          Q4<UB>::st(du, ((b * H + yo * POOL + (q / POOL)) * W + xo * POOL + (q % POOL)) * C4 + cg, rr);
        }
      }
  }
}

// 1 << lg == C / 4 if the fast forms apply to this shape, else -1
inline int v4_log2(int C, size_t elems) {
  if (C % 4 || elems >= (1ull << 31)) return -1;
  const int C4 = C / 4;
  for (int lg = 0; lg <= 6; ++lg)
    if ((1 << lg) == C4) return lg;
  return -1;
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

// =================================================================================================
// Train-mode layer pieces.  A layer of nnlib.cnn / nnlib.dcnn in training is
//   u = conv(x, w) + b                       ra_conv3x3_f32 (scale 1, shift b, no ReLU, no pool)
//   mean, var = moments(u over B,H,W)        ra_bn_moments_f32            nnlib.py:98 (biased variance)
//   y = pool(relu(gamma (u - mean) rsqrt(var + 1e-3) + beta))   ra_bn_act_pool_f32   nnlib.py:111-119,250-253
// and backward (batch statistics are part of the graph, nnlib.py:98-112):
//   dbeta, dgamma, du                        ra_bn_act_pool_bwd_f32
//   dx = conv(du, w^T flipped)               ra_conv3x3_f32 on ra_conv_pack_weights_dev(.., TRANSPOSED)
//   dw, db                                   ra_conv3x3_wgrad_f32
// All reductions are two-stage with a fixed summation order (no atomics): bit-reproducible.
namespace ra {
namespace train {

constexpr int kRedBlocks = 512;

// ---- per-channel moments: pass 1 sum, pass 2 sum of squared deviations (tf.nn.moments) ----
__global__ __launch_bounds__(256) void chan_sum_kernel(const float *u, size_t npix, int C, const float *mean,
                                                       float *part) {
  // thread = (pixel lane, channel): channel = tid % C when C divides 256; generic otherwise
  __shared__ float red[256];
  const int tid = threadIdx.x;
  const int lanes = 256 / C;  // pixel lanes per block (C <= 256, power-of-two-friendly but generic)
  const int c = tid % C, pl = tid / C;
  float s = 0.f;
  if (pl < lanes) {
    const float mu = mean ? mean[c] : 0.f;
    for (size_t p = (size_t)blockIdx.x * lanes + pl; p < npix; p += (size_t)gridDim.x * lanes) {
      const float v = u[p * C + c] - mu;
      s += mean ? v * v : v;
    }
  }
  red[tid] = pl < lanes ? s : 0.f;
  __syncthreads();
  if (tid < C) {
    float t = 0.f;
    for (int k = 0; k < lanes; ++k) t += red[k * C + tid];
    part[(size_t)blockIdx.x * C + tid] = t;
  }
}
// One workgroup per channel: 256 threads stride over the partial blocks, then a fixed-shape tree
// (deterministic); a single thread per channel walking 512 strided partials took ~60 us.
__device__ inline float block_sum256(float v, float *red) {
  const int tid = threadIdx.x;
  red[tid] = v;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  const float r = red[0];
  __syncthreads();
  return r;
}
__global__ __launch_bounds__(256) void chan_final_kernel(const float *part, int nblocks, int C, float inv_n, float *out) {
  __shared__ float red[256];
  const int c = blockIdx.x;
  float t = 0.f;
  for (int k = threadIdx.x; k < nblocks; k += 256) t += part[(size_t)k * C + c];
  t = block_sum256(t, red);
  if (threadIdx.x == 0) out[c] = t * inv_n;
}

// tf.nn.moments from the records the conv epilogue left (ra_conv3x3_moments_f32: {n, S1, S2, pivot} per channel and
// record, sums of (u - pivot) and (u - pivot)^2): one workgroup per channel and ONE pass over the records.  Every record is
// re-based in float64 onto a common reference P0 (the first record's pivot — an actual value of the channel):
//   sum (u - P0) = S1 + n d,   sum (u - P0)^2 = S2 + d (2 S1 + n d),   d = pivot - P0
// and mean = P0 + A / N, var = Q / N - (A / N)^2.  The subtraction cancels only (mean - P0)^2 against the spread — a few
// sigma^2 at most, 53 bits under it — not the E[x^2] - E[x]^2 of raw float32 sums.
template <int NT>  // threads per channel: 64 (one wave, no barrier) up to 512 records, else 256
__global__ __launch_bounds__(NT) void moments_from_partials_kernel(const float *part, int nparts, int C, int CP, float *mean,
                                                                   float *var) {
  __shared__ double red[3][NT / 64];
  const int c = blockIdx.x, tid = threadIdx.x;
  const f32x4 r0 = *reinterpret_cast<const f32x4 *>(part + (size_t)c * 4);
  const double P0 = r0[0] > 0.f ? (double)r0[3] : 0.0;
  double n = 0.0, sa = 0.0, sq = 0.0;
  for (int k = tid; k < nparts; k += NT) {
    const f32x4 r = *reinterpret_cast<const f32x4 *>(part + ((size_t)k * CP + c) * 4);
    if (r[0] > 0.f) {
      const double d = (double)r[3] - P0, nd = (double)r[0] * d;
      n += (double)r[0];
      sa += (double)r[1] + nd;
      sq += (double)r[2] + d * (2.0 * (double)r[1] + nd);
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    n += __shfl_xor(n, o, 64);
    sa += __shfl_xor(sa, o, 64);
    sq += __shfl_xor(sq, o, 64);
  }
  if constexpr (NT > 64) {
    if ((tid & 63) == 0) red[0][tid >> 6] = n, red[1][tid >> 6] = sa, red[2][tid >> 6] = sq;
    __syncthreads();
    n = sa = sq = 0.0;
#pragma unroll
    for (int w = 0; w < NT / 64; ++w) n += red[0][w], sa += red[1][w], sq += red[2][w];
  }
  if (tid == 0) {
    const double N = n > 0.0 ? n : 1.0, a = sa / N, v = sq / N - a * a;
    mean[c] = (float)(P0 + a);
    var[c] = (float)(v > 0.0 ? v : 0.0);
  }
}

// ---- y = pool(relu(gamma * (u - mean) * rstd + beta)) ----
__global__ __launch_bounds__(256) void bn_act_pool_kernel(const float *u, const float *mean, const float *var,
                                                          const float *gamma, const float *beta, float eps, int relu,
                                                          int pool, int B, int H, int W, int C, float *y) {
  const int Ho = H / pool, Wo = W / pool;
  const size_t total = (size_t)B * Ho * Wo * C;
  const float lo = relu ? 0.f : -__builtin_inff();
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
    const int c = (int)(e % C);
    size_t r = e / C;
    const int xo = (int)(r % Wo);
    r /= Wo;
    const int yo = (int)(r % Ho), b = (int)(r / Ho);
    // (u - mean) first: the folded form u * g + (beta - mean * g) cancels badly in channels whose
    // mean is large against their spread, and rstd amplifies that error layer after layer
    const float g = (gamma ? gamma[c] : 1.f) * (var ? rsqrtf(var[c] + eps) : 1.f);
    const float mu = mean ? mean[c] : 0.f, be = beta ? beta[c] : 0.f;
    float best = -__builtin_inff();
    for (int dy = 0; dy < pool; ++dy)
      for (int dx = 0; dx < pool; ++dx) {
        const float v = (u[(((size_t)b * H + yo * pool + dy) * W + xo * pool + dx) * C + c] - mu) * g + be;
        best = fmaxf(best, fmaxf(v, lo));
      }
    y[e] = best;
  }
}

// ---- backward, stage 1: per-channel sums of dv and dv * xhat (dv = dy routed through pool + ReLU) ----
__device__ inline void bwd_point(const float *u, const float *dy, float g, float be, float mu, float rstd, float lo,
                                 int relu, int pool, int b, int yy, int xx, int H, int W, int C, int c, float &dv,
                                 float &xhat) {
  // gradient reaching pre-activation v at conv pixel (yy, xx): the pooled window's FIRST maximum gets dy
  const float uv = u[(((size_t)b * H + yy) * W + xx) * C + c];
  xhat = (uv - mu) * rstd;
  const float v = (uv - mu) * g + be;
  if (pool == 1) {
    dv = (relu && v <= 0.f) ? 0.f : dy[(((size_t)b * H + yy) * W + xx) * C + c];
    return;
  }
  const int yo = yy >> 1, xo = xx >> 1, Ho = H >> 1, Wo = W >> 1;
  float best = -__builtin_inff();
  int arg = 0;
  for (int k = 0; k < 4; ++k) {
    const float w = (u[(((size_t)b * H + 2 * yo + (k >> 1)) * W + 2 * xo + (k & 1)) * C + c] - mu) * g + be;
    const float a = fmaxf(w, lo);
    if (a > best) {
      best = a;
      arg = k;
    }
  }
  const bool mine = arg == (((yy & 1) << 1) | (xx & 1));
  dv = (mine && !(relu && v <= 0.f)) ? dy[(((size_t)b * Ho + yo) * Wo + xo) * C + c] : 0.f;
}

__global__ __launch_bounds__(256) void bn_bwd_reduce_kernel(const float *u, const float *dy, const float *mean,
                                                            const float *var, const float *gamma, const float *beta,
                                                            float eps, int relu, int pool, int B, int H, int W, int C,
                                                            float *part) {
  __shared__ float r0[256], r1[256];
  const int tid = threadIdx.x, lanes = 256 / C, c = tid % C, pl = tid / C;
  float s0 = 0.f, s1 = 0.f;
  if (pl < lanes) {
    const float rstd = var ? rsqrtf(var[c] + eps) : 1.f, mu = mean ? mean[c] : 0.f;
    const float g = (gamma ? gamma[c] : 1.f) * rstd, sh = beta ? beta[c] : 0.f;
    const float lo = relu ? 0.f : -__builtin_inff();
    const size_t npix = (size_t)B * H * W;
    for (size_t p = (size_t)blockIdx.x * lanes + pl; p < npix; p += (size_t)gridDim.x * lanes) {
      const int xx = (int)(p % W);
      const size_t r = p / W;
      const int yy = (int)(r % H), b = (int)(r / H);
      float dv, xhat;
      bwd_point(u, dy, g, sh, mu, rstd, lo, relu, pool, b, yy, xx, H, W, C, c, dv, xhat);
      s0 += dv;
      s1 += dv * xhat;
    }
  }
  r0[tid] = pl < lanes ? s0 : 0.f;
  r1[tid] = pl < lanes ? s1 : 0.f;
  __syncthreads();
  if (tid < C) {
    float t0 = 0.f, t1 = 0.f;
    for (int k = 0; k < lanes; ++k) {
      t0 += r0[k * C + tid];
      t1 += r1[k * C + tid];
    }
    part[((size_t)blockIdx.x * 2) * C + tid] = t0;
    part[((size_t)blockIdx.x * 2 + 1) * C + tid] = t1;
  }
}
__global__ __launch_bounds__(256) void bn_bwd_final_kernel(const float *part, int nblocks, int C, float *dbeta, float *dgamma,
                                                           float *acc_beta = nullptr, float *acc_gamma = nullptr,
                                                           float *const *tabs = nullptr, int G = 1) {
  __shared__ float red[256];
  const int c = blockIdx.x;
  if (tabs) {
    const int g = blockIdx.y;
    part += (size_t)g * nblocks * 2 * C;
    dbeta += (size_t)g * C;
    dgamma += (size_t)g * C;
    acc_gamma = tabs[4 * G + g], acc_beta = tabs[5 * G + g];
  }
  float t0 = 0.f, t1 = 0.f;
  for (int k = threadIdx.x; k < nblocks; k += 256) {
    t0 += part[((size_t)k * 2) * C + c];
    t1 += part[((size_t)k * 2 + 1) * C + c];
  }
  t0 = block_sum256(t0, red);
  t1 = block_sum256(t1, red);
  if (threadIdx.x == 0) {
    dbeta[c] = t0;
    dgamma[c] = t1;
    if (acc_beta) acc_beta[c] += t0;    // straight into the gradient bucket (one writer per element)
    if (acc_gamma) acc_gamma[c] += t1;
  }
}
// ---- stage 2: du = gamma * rstd * (dv - dbeta / n - xhat * dgamma / n)   (batch-norm: var given)
//               du = dv                                                    (no BN)
__global__ __launch_bounds__(256) void bn_bwd_dx_kernel(const float *u, const float *dy, const float *mean,
                                                        const float *var, const float *gamma, const float *beta,
                                                        const float *dbeta, const float *dgamma, float eps, int relu,
                                                        int pool, int B, int H, int W, int C, float *du, float inv_n) {
  const size_t total = (size_t)B * H * W * C;
  const float lo = relu ? 0.f : -__builtin_inff();
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
    const int c = (int)(e % C);
    size_t r = e / C;
    const int xx = (int)(r % W);
    r /= W;
    const int yy = (int)(r % H), b = (int)(r / H);
    const float rstd = var ? rsqrtf(var[c] + eps) : 1.f, mu = mean ? mean[c] : 0.f;
    const float g = (gamma ? gamma[c] : 1.f) * rstd, sh = beta ? beta[c] : 0.f;
    float dv, xhat;
    bwd_point(u, dy, g, sh, mu, rstd, lo, relu, pool, b, yy, xx, H, W, C, c, dv, xhat);
    du[e] = var ? g * (dv - dbeta[c] * inv_n - xhat * dgamma[c] * inv_n) : dv;
  }
}

// ---- small tensors (the one-channel output layer of the deconvolution net: B x 48 x 48 values per timestep): the
// whole BatchNorm backward of a call — both sums, dbeta / dgamma and du — in ONE workgroup per call; G calls (a layer's
// timesteps) = G workgroups of one launch.  1024 % C == 0 keeps a thread on one channel; fixed-shape LDS tree.
constexpr int kSmallThreads = 1024;
constexpr size_t kSmallElems = 65536;  // per group
inline bool small_ok(int C, size_t elems, int which = 1) {
  static const int on = env_int("RA_BN_SMALL", 1);  // =0: the multi-launch forms; 2: only the moments, 3: only the backward (debugging aids)
  return (on == 1 || on == which) && C >= 1 && C <= 64 && (C & (C - 1)) == 0 && elems <= kSmallElems;
}
__global__ __launch_bounds__(kSmallThreads) void bn_bwd_small_kernel(const float *u, const float *dy, const float *mean, const float *var,
                                                                    const float *gamma, const float *beta, float eps, int relu, int pool,
                                                                    int B, int H, int W, int C, float *dbeta, float *dgamma,
                                                                    float *acc_beta, float *acc_gamma, float *du, float inv_n,
                                                                    const float *const *tabs, int G) {
  __shared__ float r0[kSmallThreads], r1[kSmallThreads];
  const int g_ = blockIdx.x, tid = threadIdx.x, c = tid % C;
  const size_t total = (size_t)B * H * W * C;
  if (tabs) {
    mean = tabs[g_], var = tabs[G + g_], gamma = tabs[2 * G + g_], beta = tabs[3 * G + g_];
    acc_gamma = const_cast<float *>(tabs[4 * G + g_]), acc_beta = const_cast<float *>(tabs[5 * G + g_]);
    u += (size_t)g_ * total;
    dy += (size_t)g_ * (total / (pool * pool));
    du += (size_t)g_ * total;
    dbeta += (size_t)g_ * C, dgamma += (size_t)g_ * C;
  }
  const float rstd = var ? rsqrtf(var[c] + eps) : 1.f, mu = mean ? mean[c] : 0.f;
  const float g = (gamma ? gamma[c] : 1.f) * rstd, sh = beta ? beta[c] : 0.f;
  const float lo = relu ? 0.f : -__builtin_inff();
  float s0 = 0.f, s1 = 0.f;
  for (size_t e = tid; e < total; e += kSmallThreads) {
    size_t r = e / C;
    const int xx = (int)(r % W);
    r /= W;
    const int yy = (int)(r % H), b = (int)(r / H);
    float dv, xhat;
    bwd_point(u, dy, g, sh, mu, rstd, lo, relu, pool, b, yy, xx, H, W, C, c, dv, xhat);
    s0 += dv;
    s1 += dv * xhat;
  }
  r0[tid] = s0, r1[tid] = s1;
  __syncthreads();
  for (int o = kSmallThreads / 2; o >= C; o >>= 1) {
    if (tid < o) r0[tid] += r0[tid + o], r1[tid] += r1[tid + o];
    __syncthreads();
  }
  const float db = r0[c], dg = r1[c];
  if (tid < C) {
    dbeta[c] = db, dgamma[c] = dg;
    if (acc_beta) acc_beta[c] += db;
    if (acc_gamma) acc_gamma[c] += dg;
  }
  for (size_t e = tid; e < total; e += kSmallThreads) {
    size_t r = e / C;
    const int xx = (int)(r % W);
    r /= W;
    const int yy = (int)(r % H), b = (int)(r / H);
    float dv, xhat;
    bwd_point(u, dy, g, sh, mu, rstd, lo, relu, pool, b, yy, xx, H, W, C, c, dv, xhat);
    du[e] = var ? g * (dv - db * inv_n - xhat * dg * inv_n) : dv;
  }
}
// tf.nn.moments of a small tensor in one launch: mean, then the mean of the squared deviations about it
__global__ __launch_bounds__(kSmallThreads) void moments_small_kernel(const float *u, size_t total, int C, float inv_n, float *mean,
                                                                     float *var) {
  __shared__ float red[kSmallThreads];
  const int tid = threadIdx.x, c = tid % C;
  auto chan_sum = [&](float v) {
    red[tid] = v;
    __syncthreads();
    for (int o = kSmallThreads / 2; o >= C; o >>= 1) {
      if (tid < o) red[tid] += red[tid + o];
      __syncthreads();
    }
    const float r = red[c];
    __syncthreads();
    return r;
  };
  float s = 0.f;
  for (size_t e = tid; e < total; e += kSmallThreads) s += u[e];
  const float mu = chan_sum(s) * inv_n;
  s = 0.f;
  for (size_t e = tid; e < total; e += kSmallThreads) {
    const float d = u[e] - mu;
    s += d * d;
  }
  const float v = chan_sum(s) * inv_n;
  if (tid < C) mean[c] = mu, var[c] = v;
}

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
typedef float f32x4 __attribute__((ext_vector_type(4)));
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
      if (wt != 0.f) g = __fadd_rn(g, __fmul_rn(wt, yb[(size_t)t * HW]));  // uniform per image
    }
    if (noise) g = __fsub_rn(g, __fmul_rn(g, noise[px]));
    const float k = knob[(size_t)b * knob_stride];
    yc = __fadd_rn(__fmul_rn(k, g), __fmul_rn(__fsub_rn(1.0f, k), yc));
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

extern "C" size_t ra_bn_workspace_floats(int C) { return (size_t)ra::train::kRedBlocks * 2 * (C > 0 ? C : 1); }

extern "C" int ra_bn_moments_f32(const float *u, size_t npix, int C, float *ws, size_t ws_floats, float *mean,
                                 float *var, void *stream) {
  if (!u || !ws || !mean || !var || npix == 0 || C <= 0) return fail(RA_E_INVALID, "ra_bn_moments_f32: bad argument");
  if (C > 256) return fail(RA_E_SHAPE, "ra_bn_moments_f32: C %d > 256", C);
  if (ws_floats < ra_bn_workspace_floats(C)) return fail(RA_E_WORKSPACE, "ra_bn_moments_f32: workspace too small");
  hipStream_t st = as_stream(stream);
  const float inv_n = 1.f / (float)npix;
  if (train::small_ok(C, npix * C, 2)) {
    hipLaunchKernelGGL(train::moments_small_kernel, dim3(1), dim3(train::kSmallThreads), 0, st, u, npix * C, C, inv_n, mean, var);
    return launch_status("ra_bn_moments_f32");
  }
  if (const int lg = train::v4_log2(C, npix * C); lg >= 0) {
    const int C4 = C / 4, n4 = (int)(npix * C4);
    int nb4 = ceil_div(n4, 256);
    if (nb4 > train::kRedBlocks) nb4 = train::kRedBlocks;
    const train::f32x4 *u4 = reinterpret_cast<const train::f32x4 *>(u);
    hipLaunchKernelGGL(train::chan_sum_v4_kernel, dim3(nb4), dim3(256), 0, st, u4, n4, C4, static_cast<const float *>(nullptr), ws);
    hipLaunchKernelGGL(train::chan_final_kernel, dim3(C), dim3(256), 0, st, ws, nb4, C, inv_n, mean);
    hipLaunchKernelGGL(train::chan_sum_v4_kernel, dim3(nb4), dim3(256), 0, st, u4, n4, C4, mean, ws);
    hipLaunchKernelGGL(train::chan_final_kernel, dim3(C), dim3(256), 0, st, ws, nb4, C, inv_n, var);
    return launch_status("ra_bn_moments_f32");
  }
  const int lanes = 256 / C;
  int nb = (int)((npix + lanes - 1) / lanes);
  if (nb > train::kRedBlocks) nb = train::kRedBlocks;
  hipLaunchKernelGGL(train::chan_sum_kernel, dim3(nb), dim3(256), 0, st, u, npix, C, static_cast<const float *>(nullptr), ws);
  hipLaunchKernelGGL(train::chan_final_kernel, dim3(C), dim3(256), 0, st, ws, nb, C, inv_n, mean);
  hipLaunchKernelGGL(train::chan_sum_kernel, dim3(nb), dim3(256), 0, st, u, npix, C, mean, ws);
  hipLaunchKernelGGL(train::chan_final_kernel, dim3(C), dim3(256), 0, st, ws, nb, C, inv_n, var);
  return launch_status("ra_bn_moments_f32");
}

extern "C" int ra_bn_moments_from_partials_f32(const float *part, int nparts, int C, float *mean, float *var, void *stream) {
  const int cp = ra_conv_cout_padded(C);
  if (!part || !mean || !var || nparts <= 0 || C <= 0 || !cp) return fail(RA_E_INVALID, "ra_bn_moments_from_partials_f32: bad argument");
  if (nparts <= 512)
    hipLaunchKernelGGL(train::moments_from_partials_kernel<64>, dim3(C), dim3(64), 0, as_stream(stream), part, nparts, C, cp, mean, var);
  else  // 1024 threads measured slower than 256 at 4096 records (6.4 against ~5.1 us): the launch, not the loop
    hipLaunchKernelGGL(train::moments_from_partials_kernel<256>, dim3(C), dim3(256), 0, as_stream(stream), part, nparts, C, cp, mean, var);
  return launch_status("ra_bn_moments_from_partials_f32");
}

namespace {
template <int POOL, bool UB, bool YB>
void launch_bn_act_pool_v4(dim3 g4, hipStream_t st, const void *u, const float *mean, const float *var, const float *gamma,
                           const float *beta, float eps, int relu, int B, int H, int W, int C4, int lg, void *y) {
  hipLaunchKernelGGL((train::bn_act_pool_v4_kernel<POOL, UB, YB>), g4, dim3(256), 0, st,
                     reinterpret_cast<const typename train::Q4<UB>::T *>(u), mean, var, gamma, beta, eps, relu, B, H, W, C4, lg,
                     reinterpret_cast<typename train::Q4<YB>::T *>(y));
}
// flags: bit 0 = u is stored as bf16, bit 1 = y is written as bf16 (only combinations the bf16 mode produces: 0, 1, 3)
int bn_act_pool_impl(const void *u, const float *mean, const float *var, const float *gamma, const float *beta, float eps, int relu,
                     int pool, int B, int H, int W, int C, void *y, int flags, void *stream) {
  if (!u || !y || B <= 0 || H <= 0 || W <= 0 || C <= 0) return fail(RA_E_INVALID, "ra_bn_act_pool_f32: bad argument");
  if ((pool != 1 && pool != 2) || (pool == 2 && ((H | W) & 1))) return fail(RA_E_SHAPE, "ra_bn_act_pool_f32: pool");
  if (const int lg = train::v4_log2(C, (size_t)B * H * W * C); lg >= 0) {
    const int C4 = C / 4, rows = B * (H / pool);
    const int ry = ceil_div(rows, pool == 1 ? train::kRowsPerIter<1> : train::kRowsPerIter<2>);
    const dim3 g4(ceil_div((W / pool) * C4, 256), ry < 16384 ? ry : 16384);
    hipStream_t st = as_stream(stream);
#define RA_BNF(P, UB, YB) launch_bn_act_pool_v4<P, UB, YB>(g4, st, u, mean, var, gamma, beta, eps, relu, B, H, W, C4, lg, y)
    if (flags == 0) { if (pool == 2) RA_BNF(2, false, false); else RA_BNF(1, false, false); }
    else if (flags == 1) { if (pool == 2) RA_BNF(2, true, false); else RA_BNF(1, true, false); }
    else if (flags == 3) { if (pool == 2) RA_BNF(2, true, true); else RA_BNF(1, true, true); }
    else return fail(RA_E_INVALID, "ra_bn_act_pool_bf16_f32: flags %d", flags);
#undef RA_BNF
    return launch_status("ra_bn_act_pool_f32");
  }
  if (flags) return fail(RA_E_SHAPE, "ra_bn_act_pool_bf16_f32: bf16 storage needs C %% 4 == 0 with C / 4 a power of two (C %d)", C);
  return -1000;  // the generic float32 kernel (the caller below)
}
}  // namespace

extern "C" int ra_bn_act_pool_bf16_f32(const void *u, const float *mean, const float *var, const float *gamma, const float *beta,
                                       float eps, int relu, int pool, int B, int H, int W, int C, void *y, int flags, void *stream) {
  const int rc = bn_act_pool_impl(u, mean, var, gamma, beta, eps, relu, pool, B, H, W, C, y, flags, stream);
  if (rc != -1000) return rc;
  return ra_bn_act_pool_f32(static_cast<const float *>(u), mean, var, gamma, beta, eps, relu, pool, B, H, W, C, static_cast<float *>(y), stream);
}

extern "C" int ra_bn_act_pool_f32(const float *u, const float *mean, const float *var, const float *gamma,
                                  const float *beta, float eps, int relu, int pool, int B, int H, int W, int C, float *y,
                                  void *stream) {
  {
    const int rc = bn_act_pool_impl(u, mean, var, gamma, beta, eps, relu, pool, B, H, W, C, y, 0, stream);
    if (rc != -1000) return rc;
  }
  const size_t total = (size_t)B * (H / pool) * (W / pool) * C;
  size_t grid = (total + 255) / 256;
  if (grid > 8192) grid = 8192;
  hipLaunchKernelGGL(train::bn_act_pool_kernel, dim3((unsigned)grid), dim3(256), 0, as_stream(stream), u, mean, var, gamma,
                     beta, eps, relu, pool, B, H, W, C, y);
  return launch_status("ra_bn_act_pool_f32");
}

namespace {
// stages: 1 = the two reductions (dbeta, dgamma over THIS call's pixels), 2 = du from dbeta / dgamma and the count
// they were summed over (n_total; 0 = this call's B*H*W).  Data-parallel training with whole-batch statistics
// runs stage 1, all-reduces the 2C sums, then stage 2 with the global count (ra_train.ConvBNActPool).
// the v4 kernels of one (or G stacked) BatchNorm backward call(s), for one storage format (UB: u and du bf16, DB: dy bf16)
template <int POOL, bool UB, bool DB>
void launch_bn_bwd_v4(int stages, dim3 gr, dim3 gd, hipStream_t st, const void *u, const void *dy, const float *mean, const float *var,
                      const float *gamma, const float *beta, float eps, int relu, int B, int H, int W, int C, int C4, int lg, float *ws,
                      int nblk, float *dbeta, float *dgamma, float *acc_beta, float *acc_gamma, void *du, float inv_n,
                      const float *const *ct = nullptr, float *const *mt = nullptr, int G = 1) {
  typedef typename train::Q4<UB>::T TU;
  typedef typename train::Q4<DB>::T TD;
  const TU *u4 = reinterpret_cast<const TU *>(u);
  const TD *dy4 = reinterpret_cast<const TD *>(dy);
  if (stages & 1) {
    hipLaunchKernelGGL((train::bn_bwd_reduce_v4_kernel<POOL, UB, DB>), gr, dim3(256), 0, st, u4, dy4, mean, var, gamma, beta, eps, relu, B,
                       H, W, C4, lg, ws, ct, G);
    if (ct)
      hipLaunchKernelGGL(train::bn_bwd_final_kernel, dim3(C, G), dim3(256), 0, st, ws, nblk, C, dbeta, dgamma, (float *)nullptr,
                         (float *)nullptr, mt, G);
    else
      hipLaunchKernelGGL(train::bn_bwd_final_kernel, dim3(C), dim3(256), 0, st, ws, nblk, C, dbeta, dgamma, acc_beta, acc_gamma);
  }
  if (stages & 2)
    hipLaunchKernelGGL((train::bn_bwd_dx_v4_kernel<POOL, UB, DB>), gd, dim3(256), 0, st, u4, dy4, mean, var, gamma, beta, dbeta, dgamma,
                       eps, relu, B, H, W, C4, lg, reinterpret_cast<TU *>(du), inv_n, ct, G);
}
template <typename... A>
int dispatch_bn_bwd_v4(int pool, int flags, A... a) {
  if (flags == 0) { if (pool == 2) launch_bn_bwd_v4<2, false, false>(a...); else launch_bn_bwd_v4<1, false, false>(a...); }
  else if (flags == 1) { if (pool == 2) launch_bn_bwd_v4<2, true, false>(a...); else launch_bn_bwd_v4<1, true, false>(a...); }
  else if (flags == 3) { if (pool == 2) launch_bn_bwd_v4<2, true, true>(a...); else launch_bn_bwd_v4<1, true, true>(a...); }
  else return fail(RA_E_INVALID, "ra_bn_act_pool_bwd: storage flags %d", flags);
  return 0;
}

int bn_bwd_impl(const float *u, const float *dy, const float *mean, const float *var, const float *gamma,
                const float *beta, float eps, int relu, int pool, int B, int H, int W, int C, float *ws,
                size_t ws_floats, float *dgamma, float *dbeta, float *du, float *acc_gamma, float *acc_beta,
                void *stream, int stages = 3, double n_total = 0.0, int flags = 0) {
  if (!u || !dy || !dgamma || !dbeta || ((stages & 1) && !ws) || ((stages & 2) && !du) || B <= 0 || H <= 0 || W <= 0 || C <= 0)
    return fail(RA_E_INVALID, "ra_bn_act_pool_bwd_f32: bad argument");
  if (C > 256) return fail(RA_E_SHAPE, "ra_bn_act_pool_bwd_f32: C %d > 256", C);
  if ((pool != 1 && pool != 2) || (pool == 2 && ((H | W) & 1))) return fail(RA_E_SHAPE, "ra_bn_act_pool_bwd_f32: pool");
  if ((stages & 1) && ws_floats < ra_bn_workspace_floats(C)) return fail(RA_E_WORKSPACE, "ra_bn_act_pool_bwd_f32: workspace too small");
  hipStream_t st = as_stream(stream);
  const size_t npix = (size_t)B * H * W;
  const float inv_n = (float)(1.0 / (n_total > 0.0 ? n_total : (double)npix));
  if (const int lg = train::v4_log2(C, npix * C); lg >= 0 && ceil_div((W / pool) * (C / 4), 256) <= train::kRedBlocks) {
    const int C4 = C / 4, rows = B * (H / pool), gx = ceil_div((W / pool) * C4, 256);
    int gy = train::kRedBlocks / gx;
    if (gy > rows) gy = rows;
    const int ry = ceil_div(rows, pool == 1 ? train::kRowsPerIter<1> : train::kRowsPerIter<2>);
    const dim3 gr(gx, gy), gd(gx, ry < 16384 ? ry : 16384);
    if (const int rc = dispatch_bn_bwd_v4(pool, flags, stages, gr, gd, st, (const void *)u, (const void *)dy, mean, var, gamma, beta, eps, relu,
                                          B, H, W, C, C4, lg, ws, gx * gy, dbeta, dgamma, acc_beta, acc_gamma, (void *)du, inv_n,
                                          (const float *const *)nullptr, (float *const *)nullptr, 1))
      return rc;
    return launch_status("ra_bn_act_pool_bwd_f32");
  }
  if (flags) return fail(RA_E_SHAPE, "ra_bn_act_pool_bwd: bf16 storage needs C %% 4 == 0 with C / 4 a power of two (C %d)", C);
  if (stages == 3 && train::small_ok(C, npix * C, 3)) {
    hipLaunchKernelGGL(train::bn_bwd_small_kernel, dim3(1), dim3(train::kSmallThreads), 0, st, u, dy, mean, var, gamma, beta, eps, relu,
                       pool, B, H, W, C, dbeta, dgamma, acc_beta, acc_gamma, du, inv_n, (const float *const *)nullptr, 1);
    return launch_status("ra_bn_act_pool_bwd_f32");
  }
  const int lanes = 256 / C;
  int nb = (int)((npix + lanes - 1) / lanes);
  if (nb > train::kRedBlocks) nb = train::kRedBlocks;
  if (stages & 1) {
    hipLaunchKernelGGL(train::bn_bwd_reduce_kernel, dim3(nb), dim3(256), 0, st, u, dy, mean, var, gamma, beta, eps, relu, pool,
                       B, H, W, C, ws);
    hipLaunchKernelGGL(train::bn_bwd_final_kernel, dim3(C), dim3(256), 0, st, ws, nb, C, dbeta, dgamma, acc_beta, acc_gamma);
  }
  if (stages & 2) {
    size_t grid = (npix * C + 255) / 256;
    if (grid > 8192) grid = 8192;
    hipLaunchKernelGGL(train::bn_bwd_dx_kernel, dim3((unsigned)grid), dim3(256), 0, st, u, dy, mean, var, gamma, beta, dbeta,
                       dgamma, eps, relu, pool, B, H, W, C, du, inv_n);
  }
  return launch_status("ra_bn_act_pool_bwd_f32");
}
}  // namespace

// G calls of one BatchNorm layer (its G timesteps) stacked along the batch — u [G*B,H,W,C], dy [G*B,H/pool,W/pool,C] — in
// one reduce / final / dx triple: every group has its own statistics and parameters, read through a device table of
// 6 G pointers {mean, var, gamma, beta, grad-bucket gamma, grad-bucket beta}[G]; dgamma / dbeta [G,C].
static int bn_bwd_grouped_impl(const void *u, const void *dy, const void *const *tabs, int G, float eps, int relu, int pool, int B,
                               int H, int W, int C, float *ws, size_t ws_floats, float *dgamma, float *dbeta, void *du, int flags,
                               void *stream) {
  if (!u || !dy || !tabs || !ws || !dgamma || !dbeta || !du || G <= 0 || B <= 0 || H <= 0 || W <= 0 || C <= 0)
    return fail(RA_E_INVALID, "ra_bn_act_pool_bwd_grouped_f32: bad argument");
  if ((pool != 1 && pool != 2) || (pool == 2 && ((H | W) & 1))) return fail(RA_E_SHAPE, "ra_bn_act_pool_bwd_grouped_f32: pool");
  if (ws_floats < (size_t)G * ra_bn_workspace_floats(C)) return fail(RA_E_WORKSPACE, "ra_bn_act_pool_bwd_grouped_f32: workspace too small");
  const size_t npix = (size_t)B * H * W;
  const int lg = train::v4_log2(C, npix * C);
  if (lg < 0 && flags == 0 && G <= 65535 && train::small_ok(C, npix * C, 3)) {  // one workgroup per group (the one-channel output layer)
    hipLaunchKernelGGL(train::bn_bwd_small_kernel, dim3(G), dim3(train::kSmallThreads), 0, as_stream(stream), static_cast<const float *>(u),
                       static_cast<const float *>(dy), (const float *)nullptr, (const float *)nullptr, (const float *)nullptr,
                       (const float *)nullptr, eps, relu, pool, B, H, W, C, dbeta, dgamma, (float *)nullptr, (float *)nullptr,
                       static_cast<float *>(du), (float)(1.0 / (double)npix), reinterpret_cast<const float *const *>(tabs), G);
    return launch_status("ra_bn_act_pool_bwd_grouped_f32");
  }
  if (lg < 0 || ceil_div((W / pool) * (C / 4), 256) > train::kRedBlocks || G > 65535)
    return fail(RA_E_SHAPE, "ra_bn_act_pool_bwd_grouped_f32: C %d (needs C %% 4 == 0, C / 4 a power of two <= 64)", C);
  hipStream_t st = as_stream(stream);
  const float inv_n = (float)(1.0 / (double)npix);
  const int C4 = C / 4, rows = B * (H / pool), gx = ceil_div((W / pool) * C4, 256);
  int gy = train::kRedBlocks / gx;
  if (gy > rows) gy = rows;
  const float *const *ct = reinterpret_cast<const float *const *>(tabs);
  float *const *mt = reinterpret_cast<float *const *>(const_cast<void *const *>(tabs));
  const int ry = ceil_div(rows, pool == 1 ? train::kRowsPerIter<1> : train::kRowsPerIter<2>);
  const dim3 gr(gx, gy, G), gd(gx, ry < 16384 ? ry : 16384, G);
  const float *nul = nullptr;
  if (const int rc = dispatch_bn_bwd_v4(pool, flags, 3, gr, gd, st, u, dy, nul, nul, nul, nul, eps, relu, B, H, W, C, C4, lg, ws, gx * gy,
                                        dbeta, dgamma, (float *)nullptr, (float *)nullptr, du, inv_n, ct, mt, G))
    return rc;
  return launch_status("ra_bn_act_pool_bwd_grouped_f32");
}

extern "C" int ra_bn_act_pool_bwd_grouped_f32(const float *u, const float *dy, const void *const *tabs, int G, float eps, int relu,
                                              int pool, int B, int H, int W, int C, float *ws, size_t ws_floats, float *dgamma,
                                              float *dbeta, float *du, void *stream) {
  return bn_bwd_grouped_impl(u, dy, tabs, G, eps, relu, pool, B, H, W, C, ws, ws_floats, dgamma, dbeta, du, 0, stream);
}

// The bf16 mode's forms (model_opt['compute_dtype'] = 'bf16'): flags bit 0 = u is read and du written as bf16, bit 1 = dy is
// read as bf16 (0, 1 or 3); float32 statistics, sums and parameter gradients.
extern "C" int ra_bn_act_pool_bwd_grouped_bf16_f32(const void *u, const void *dy, const void *const *tabs, int G, float eps, int relu,
                                                   int pool, int B, int H, int W, int C, float *ws, size_t ws_floats, float *dgamma,
                                                   float *dbeta, void *du, int flags, void *stream) {
  return bn_bwd_grouped_impl(u, dy, tabs, G, eps, relu, pool, B, H, W, C, ws, ws_floats, dgamma, dbeta, du, flags, stream);
}

extern "C" int ra_bn_act_pool_bwd_acc_bf16_f32(const void *u, const void *dy, const float *mean, const float *var, const float *gamma,
                                               const float *beta, float eps, int relu, int pool, int B, int H, int W, int C, float *ws,
                                               size_t ws_floats, float *dgamma, float *dbeta, void *du, float *acc_gamma,
                                               float *acc_beta, int flags, void *stream) {
  return bn_bwd_impl(static_cast<const float *>(u), static_cast<const float *>(dy), mean, var, gamma, beta, eps, relu, pool, B, H, W, C, ws,
                     ws_floats, dgamma, dbeta, static_cast<float *>(du), acc_gamma, acc_beta, stream, 3, 0.0, flags);
}

extern "C" int ra_bn_act_pool_bwd_f32(const float *u, const float *dy, const float *mean, const float *var,
                                      const float *gamma, const float *beta, float eps, int relu, int pool, int B,
                                      int H, int W, int C, float *ws, size_t ws_floats, float *dgamma, float *dbeta,
                                      float *du, void *stream) {
  return bn_bwd_impl(u, dy, mean, var, gamma, beta, eps, relu, pool, B, H, W, C, ws, ws_floats, dgamma, dbeta, du, nullptr,
                     nullptr, stream);
}

extern "C" int ra_bn_act_pool_bwd_acc_f32(const float *u, const float *dy, const float *mean, const float *var,
                                          const float *gamma, const float *beta, float eps, int relu, int pool, int B,
                                          int H, int W, int C, float *ws, size_t ws_floats, float *dgamma, float *dbeta,
                                          float *du, float *acc_gamma, float *acc_beta, void *stream) {
  return bn_bwd_impl(u, dy, mean, var, gamma, beta, eps, relu, pool, B, H, W, C, ws, ws_floats, dgamma, dbeta, du, acc_gamma,
                     acc_beta, stream);
}

extern "C" int ra_bn_act_pool_bwd_reduce_f32(const float *u, const float *dy, const float *mean, const float *var,
                                             const float *gamma, const float *beta, float eps, int relu, int pool, int B,
                                             int H, int W, int C, float *ws, size_t ws_floats, float *dgamma, float *dbeta,
                                             float *acc_gamma, float *acc_beta, void *stream) {
  return bn_bwd_impl(u, dy, mean, var, gamma, beta, eps, relu, pool, B, H, W, C, ws, ws_floats, dgamma, dbeta, nullptr,
                     acc_gamma, acc_beta, stream, 1);
}

extern "C" int ra_bn_act_pool_bwd_dx_f32(const float *u, const float *dy, const float *mean, const float *var,
                                         const float *gamma, const float *beta, const float *dgamma_sum,
                                         const float *dbeta_sum, double n_total, float eps, int relu, int pool, int B, int H,
                                         int W, int C, float *du, void *stream) {
  return bn_bwd_impl(u, dy, mean, var, gamma, beta, eps, relu, pool, B, H, W, C, nullptr, 0, const_cast<float *>(dgamma_sum),
                     const_cast<float *>(dbeta_sum), du, nullptr, nullptr, stream, 2, n_total);
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
