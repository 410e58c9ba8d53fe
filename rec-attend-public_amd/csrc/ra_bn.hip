// Train-mode BatchNorm of a conv layer (nnlib.py:98-119,250-253): after u = conv(x, w) + b of nnlib.cnn / nnlib.dcnn,
//   mean, var = moments(u over B,H,W)                           ra_bn_moments_f32    nnlib.py:98 (biased variance)
//   y = pool(relu(gamma (u - mean) rsqrt(var + 1e-3) + beta))   ra_bn_act_pool_f32   nnlib.py:111-119,250-253
//   dbeta, dgamma, du                                           ra_bn_act_pool_bwd_f32 (the statistics are part of the graph)
// All reductions are two-stage with a fixed summation order (no atomics): bit-reproducible.
//
// Every pass has up to three FORMS; bn_form() below is the one place that picks among them (exported as ra_bn_form):
//   v4       a thread owns four channels of one pooling window (C % 4 == 0, C / 4 a power of two <= 64); takes bf16 storage
//   small    the whole call in ONE workgroup (at most 65536 values: the one-channel output layer of the deconvolution net)
//   generic  scalar kernels for any C <= 256
// The v4 and the scalar kernels are two implementations on the two sides of that choice and share no kernel code.
#include <type_traits>

#include "ra_common.h"
#include "ra_bn_parts.h"

namespace ra {
namespace train {

constexpr int kRedBlocks = 512;  // partial sums per channel that a reduction leaves for its finishing launch, at most
constexpr int kMaxC = 256;       // channels of the moments and of the per-call backward (a finishing workgroup per channel)
constexpr int kSmallThreads = 1024;
constexpr size_t kSmallElems = 65536;  // per group

// =================================================================================================
// Fast forms of the BatchNorm elementwise / reduction passes for C % 4 == 0 with C / 4 a power of two
// (every layer of the three CNNs except 1- or 3-channel ends): a thread owns FOUR channels of one
// pooling window — float4 loads, 32-bit indices, the window's (up to 4) pixels read once instead of
// once per pixel, the per-channel constants hoisted (the grid stride is a multiple of C / 4, so a
// thread's channel group never changes).  The generic kernels below moved 0.5 TB/s.
// Summation order is fixed (no atomics): bit-reproducible.
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

// =================================================================================================
// The scalar kernels: generic (any C <= 256, thread = (pixel lane, channel)) and one-workgroup ("small").  What they share:
// the constants of one channel,
struct ChanConst {
  float rstd, mu, g, sh, lo;  // lo: the floor of the activation (0 with ReLU, -inf without)
};
__device__ inline ChanConst chan_const(const float *mean, const float *var, const float *gamma, const float *beta, float eps,
                                       int relu, int c) {
  ChanConst k;
  k.rstd = var ? rsqrtf(var[c] + eps) : 1.f;
  k.mu = mean ? mean[c] : 0.f;
  k.g = (gamma ? gamma[c] : 1.f) * k.rstd;
  k.sh = beta ? beta[c] : 0.f;
  k.lo = relu ? 0.f : -__builtin_inff();
  return k;
}
// the pixel of a row-major index over [B, H, W] (an element index e over [B, H, W, C] is pixel e / C, channel e % C),
struct Pixel {
  int b, y, x;
};
__device__ inline Pixel pixel_of(size_t p, int H, int W) {
  const int x = (int)(p % W);
  p /= W;
  return Pixel{(int)(p / H), (int)(p % H), x};
}
// the sums a generic reduction's thread tid < C takes over its channel's column of N arrays [pixel lane][C], lane after lane,
template <int N>
__device__ inline void lds_column_sums(const float (&red)[N][256], int C, int lanes, float (&t)[N]) {
#pragma unroll
  for (int i = 0; i < N; ++i) t[i] = 0.f;
  for (int k = 0; k < lanes; ++k) {
#pragma unroll
    for (int i = 0; i < N; ++i) t[i] += red[i][k * C + threadIdx.x];
  }
}
// and the one-workgroup kernels' sums over the threads that share tid % C (kSmallThreads % C == 0 keeps a thread on one
// channel), N at a time in a fixed-shape LDS tree, left in every thread.  red is free again after the caller's next barrier.
template <int N>
__device__ inline void small_chan_sums(float (&v)[N], float (&red)[N][kSmallThreads], int C) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int i = 0; i < N; ++i) red[i][tid] = v[i];
  __syncthreads();
  for (int o = kSmallThreads / 2; o >= C; o >>= 1) {
    if (tid < o) {
#pragma unroll
      for (int i = 0; i < N; ++i) red[i][tid] += red[i][tid + o];
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] = red[i][tid % C];
}

// ---- per-channel moments: pass 1 sum, pass 2 sum of squared deviations (tf.nn.moments) ----
__global__ __launch_bounds__(256) void chan_sum_kernel(const float *u, size_t npix, int C, const float *mean,
                                                       float *part) {
  // thread = (pixel lane, channel): channel = tid % C when C divides 256; generic otherwise
  __shared__ float red[1][256];
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
  red[0][tid] = pl < lanes ? s : 0.f;
  __syncthreads();
  if (tid < C) {
    float t[1];
    lds_column_sums(red, C, lanes, t);
    part[(size_t)blockIdx.x * C + tid] = t[0];
  }
}
// One workgroup per channel: 256 threads stride over the partial blocks, then a fixed-shape tree
// (block_sum256: deterministic); a single thread per channel walking 512 strided partials took ~60 us.
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
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
    const int c = (int)(e % C);
    const Pixel o = pixel_of(e / C, Ho, Wo);
    // (u - mean) first: the folded form u * g + (beta - mean * g) cancels badly in channels whose
    // mean is large against their spread, and rstd amplifies that error layer after layer
    const ChanConst k = chan_const(mean, var, gamma, beta, eps, relu, c);
    float best = -__builtin_inff();
    for (int dy = 0; dy < pool; ++dy)
      for (int dx = 0; dx < pool; ++dx) {
        const float v = (u[(((size_t)o.b * H + o.y * pool + dy) * W + o.x * pool + dx) * C + c] - k.mu) * k.g + k.sh;
        best = fmaxf(best, fmaxf(v, k.lo));
      }
    y[e] = best;
  }
}

// ---- backward, stage 1: per-channel sums of dv and dv * xhat (dv = dy routed through pool + ReLU) ----
__device__ inline void bwd_point(const float *u, const float *dy, const ChanConst &k, int relu, int pool, Pixel p, int H, int W,
                                 int C, int c, float &dv, float &xhat) {
  // gradient reaching pre-activation v at conv pixel (yy, xx): the pooled window's FIRST maximum gets dy
  const int b = p.b, yy = p.y, xx = p.x;
  const float uv = u[(((size_t)b * H + yy) * W + xx) * C + c];
  xhat = (uv - k.mu) * k.rstd;
  const float v = (uv - k.mu) * k.g + k.sh;
  if (pool == 1) {
    dv = (relu && v <= 0.f) ? 0.f : dy[(((size_t)b * H + yy) * W + xx) * C + c];
    return;
  }
  const int yo = yy >> 1, xo = xx >> 1, Ho = H >> 1, Wo = W >> 1;
  float best = -__builtin_inff();
  int arg = 0;
  for (int q = 0; q < 4; ++q) {
    const float w = (u[(((size_t)b * H + 2 * yo + (q >> 1)) * W + 2 * xo + (q & 1)) * C + c] - k.mu) * k.g + k.sh;
    const float a = fmaxf(w, k.lo);
    if (a > best) {
      best = a;
      arg = q;
    }
  }
  const bool mine = arg == (((yy & 1) << 1) | (xx & 1));
  dv = (mine && !(relu && v <= 0.f)) ? dy[(((size_t)b * Ho + yo) * Wo + xo) * C + c] : 0.f;
}

__global__ __launch_bounds__(256) void bn_bwd_reduce_kernel(const float *u, const float *dy, const float *mean,
                                                            const float *var, const float *gamma, const float *beta,
                                                            float eps, int relu, int pool, int B, int H, int W, int C,
                                                            float *part) {
  __shared__ float red[2][256];
  const int tid = threadIdx.x, lanes = 256 / C, c = tid % C, pl = tid / C;
  float s0 = 0.f, s1 = 0.f;
  if (pl < lanes) {
    const ChanConst k = chan_const(mean, var, gamma, beta, eps, relu, c);
    const size_t npix = (size_t)B * H * W;
    for (size_t p = (size_t)blockIdx.x * lanes + pl; p < npix; p += (size_t)gridDim.x * lanes) {
      float dv, xhat;
      bwd_point(u, dy, k, relu, pool, pixel_of(p, H, W), H, W, C, c, dv, xhat);
      s0 += dv;
      s1 += dv * xhat;
    }
  }
  red[0][tid] = pl < lanes ? s0 : 0.f;
  red[1][tid] = pl < lanes ? s1 : 0.f;
  __syncthreads();
  if (tid < C) {
    float t[2];
    lds_column_sums(red, C, lanes, t);
    part[((size_t)blockIdx.x * 2) * C + tid] = t[0];
    part[((size_t)blockIdx.x * 2 + 1) * C + tid] = t[1];
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
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
    const int c = (int)(e % C);
    const ChanConst k = chan_const(mean, var, gamma, beta, eps, relu, c);
    float dv, xhat;
    bwd_point(u, dy, k, relu, pool, pixel_of(e / C, H, W), H, W, C, c, dv, xhat);
    du[e] = var ? k.g * (dv - dbeta[c] * inv_n - xhat * dgamma[c] * inv_n) : dv;
  }
}

// ---- small tensors (the one-channel output layer of the deconvolution net: B x 48 x 48 values per timestep): the
// whole BatchNorm backward of a call — both sums, dbeta / dgamma and du — in ONE workgroup per call; G calls (a layer's
// timesteps) = G workgroups of one launch.  1024 % C == 0 keeps a thread on one channel; fixed-shape LDS tree.
__global__ __launch_bounds__(kSmallThreads) void bn_bwd_small_kernel(const float *u, const float *dy, const float *mean, const float *var,
                                                                    const float *gamma, const float *beta, float eps, int relu, int pool,
                                                                    int B, int H, int W, int C, float *dbeta, float *dgamma,
                                                                    float *acc_beta, float *acc_gamma, float *du, float inv_n,
                                                                    const float *const *tabs, int G) {
  __shared__ float red[2][kSmallThreads];
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
  const ChanConst k = chan_const(mean, var, gamma, beta, eps, relu, c);
  float s[2] = {0.f, 0.f};
  for (size_t e = tid; e < total; e += kSmallThreads) {
    float dv, xhat;
    bwd_point(u, dy, k, relu, pool, pixel_of(e / C, H, W), H, W, C, c, dv, xhat);
    s[0] += dv;
    s[1] += dv * xhat;
  }
  small_chan_sums(s, red, C);
  const float db = s[0], dg = s[1];
  if (tid < C) {
    dbeta[c] = db, dgamma[c] = dg;
    if (acc_beta) acc_beta[c] += db;
    if (acc_gamma) acc_gamma[c] += dg;
  }
  for (size_t e = tid; e < total; e += kSmallThreads) {
    float dv, xhat;
    bwd_point(u, dy, k, relu, pool, pixel_of(e / C, H, W), H, W, C, c, dv, xhat);
    du[e] = var ? k.g * (dv - db * inv_n - xhat * dg * inv_n) : dv;
  }
}
// tf.nn.moments of a small tensor in one launch: mean, then the mean of the squared deviations about it
__global__ __launch_bounds__(kSmallThreads) void moments_small_kernel(const float *u, size_t total, int C, float inv_n, float *mean,
                                                                     float *var) {
  __shared__ float red[1][kSmallThreads];
  const int tid = threadIdx.x, c = tid % C;
  float s[1] = {0.f};
  for (size_t e = tid; e < total; e += kSmallThreads) s[0] += u[e];
  small_chan_sums(s, red, C);
  const float mu = s[0] * inv_n;
  __syncthreads();
  s[0] = 0.f;
  for (size_t e = tid; e < total; e += kSmallThreads) {
    const float d = u[e] - mu;
    s[0] += d * d;
  }
  small_chan_sums(s, red, C);
  const float v = s[0] * inv_n;
  if (tid < C) mean[c] = mu, var[c] = v;
}

}  // namespace train
}  // namespace ra

using namespace ra;

// =================================================================================================
// Host side: one chooser, one float4 grid, one storage dispatch, one argument check.
namespace {
using train::kRedBlocks;

// 1 << lg == C / 4 if the fast forms apply to this shape, else -1
inline int v4_log2(int C, size_t elems) {
  if (C % 4 || elems >= (1ull << 31)) return -1;
  const int C4 = C / 4;
  for (int lg = 0; lg <= 6; ++lg)
    if ((1 << lg) == C4) return lg;
  return -1;
}
inline bool small_ok(int C, size_t elems) { return C >= 1 && C <= 64 && (C & (C - 1)) == 0 && elems <= train::kSmallElems; }

// The form (RA_BN_FORM_*) of one pass (RA_BN_PASS_*) over u [B,H,W,C] of npix = B H W pixels, or the RA_E_* code the entry point
// returns without a launch.  flags: the bf16 storage bits of the entry point (0 = float32 tensors); stages: of the per-call
// backward, 1 = reduce | 2 = dx; G: 0 = a per-call backward, else the groups of a grouped one.  The order of the questions
// differs per pass and is part of the contract: at C = 8 with 65536 values the moments are `small` and the backward is `v4`.
int bn_form(int pass, int C, size_t npix, int W, int pool, int flags, int stages, int G) {
  const size_t elems = npix * C;
  const bool v4 = v4_log2(C, elems) >= 0, small = small_ok(C, elems);
  // a reduction's grid is gx * gy <= kRedBlocks workgroups: the backward needs gx itself to fit
  const bool v4_bwd = v4 && ceil_div((W / pool) * (C / 4), 256) <= kRedBlocks;
  const int as_v4 = (flags == 0 || flags == 1 || flags == 3) ? RA_BN_FORM_V4 : RA_E_INVALID;  // only the float4 kernels read the bits
  switch (pass) {
    case RA_BN_PASS_MOMENTS:
      if (C > train::kMaxC) return RA_E_SHAPE;
      return small ? RA_BN_FORM_SMALL : v4 ? RA_BN_FORM_V4 : RA_BN_FORM_GENERIC;
    case RA_BN_PASS_FORWARD:
      if (v4) return as_v4;
      return flags ? RA_E_SHAPE : RA_BN_FORM_GENERIC;
    case RA_BN_PASS_BACKWARD:
      if (G > 0) {  // grouped: one workgroup per group (the one-channel output layer), or the float4 kernels with the group in grid.z
        if (!v4 && flags == 0 && G <= 65535 && small) return RA_BN_FORM_SMALL;
        return (v4_bwd && G <= 65535) ? as_v4 : RA_E_SHAPE;
      }
      if (C > train::kMaxC) return RA_E_SHAPE;
      if (v4_bwd) return as_v4;
      if (flags) return RA_E_SHAPE;
      return (stages == 3 && small) ? RA_BN_FORM_SMALL : RA_BN_FORM_GENERIC;
  }
  return RA_E_INVALID;
}
int form_error(int rc, const char *who, int C, int flags) {
  return fail(rc, "%s: no kernel form for C %d with storage flags %d (0, 1, 3; they and a grouped call need the float4 kernels)", who, C, flags);
}

// The argument check of every entry point: ok = its pointers and extents, cmax = its channel limit (0x7fffffff: none),
// ws_need = the floats of workspace it was handed ws_have for.
int check_call(const char *who, bool ok, int C, int cmax, int pool, int H, int W, size_t ws_have, size_t ws_need) {
  if (!ok || C <= 0) return fail(RA_E_INVALID, "%s: bad argument", who);
  if (C > cmax) return fail(RA_E_SHAPE, "%s: C %d > %d", who, C, cmax);
  if ((pool != 1 && pool != 2) || (pool == 2 && ((H | W) & 1))) return fail(RA_E_SHAPE, "%s: pool", who);
  if (ws_have < ws_need) return fail(RA_E_WORKSPACE, "%s: workspace too small", who);
  return 0;
}

// The grids of the float4 kernels over u [B,H,W,C]: x covers a row of (W / pool) windows x C / 4 channel quads, y the rows.
struct V4Grid {
  int C4, lg, gx, gy, ry;
  V4Grid(int C, int B, int H, int W, int pool) {
    C4 = C / 4;
    lg = 31 - __builtin_clz(C4);
    const int rows = B * (H / pool);
    gx = ceil_div((W / pool) * C4, 256);
    gy = kRedBlocks / gx < rows ? kRedBlocks / gx : rows;  // a reduction leaves gx * gy <= kRedBlocks partials per channel
    ry = ceil_div(rows, pool == 1 ? train::kRowsPerIter<1> : train::kRowsPerIter<2>);
    if (ry > 16384) ry = 16384;
  }
  int partials() const { return gx * gy; }
  dim3 reduce(int G = 1) const { return dim3(gx, gy, G); }
  dim3 elementwise(int G = 1) const { return dim3(gx, ry, G); }
};

// f(POOL, UB, XB) with the kernels' template arguments as integral constants.  flags bit 0: u (and du) stored as bf16,
// bit 1: the pass's other tensor (y forward, dy backward); the bf16 mode produces 0, 1 and 3 and bn_form refuses the rest.
template <typename F>
void with_storage(int pool, int flags, F f) {
  auto at_pool = [&](auto ub, auto xb) {
    if (pool == 2) f(std::integral_constant<int, 2>{}, ub, xb);
    else f(std::integral_constant<int, 1>{}, ub, xb);
  };
  if (flags == 0) at_pool(std::false_type{}, std::false_type{});
  else if (flags == 1) at_pool(std::true_type{}, std::false_type{});
  else at_pool(std::true_type{}, std::true_type{});
}
}  // namespace

extern "C" int ra_bn_form(int pass, int C, int B, int H, int W, int pool, int flags, int stages, int G) {
  if (pass < RA_BN_PASS_MOMENTS || pass > RA_BN_PASS_BACKWARD) return fail(RA_E_INVALID, "ra_bn_form: pass %d", pass);
  if (pass == RA_BN_PASS_MOMENTS) pool = 1;
  if (const int rc = check_call("ra_bn_form", B > 0 && H > 0 && W > 0 && G >= 0, C, 0x7fffffff, pool, H, W, 0, 0)) return rc;
  return bn_form(pass, C, (size_t)B * H * W, W, pool, flags, stages, G);
}

extern "C" size_t ra_bn_workspace_floats(int C) { return (size_t)kRedBlocks * 2 * (C > 0 ? C : 1); }

extern "C" int ra_bn_moments_f32(const float *u, size_t npix, int C, float *ws, size_t ws_floats, float *mean,
                                 float *var, void *stream) {
  const char *who = "ra_bn_moments_f32";
  if (const int rc = check_call(who, u && ws && mean && var && npix != 0, C, train::kMaxC, 1, 0, 0, ws_floats, ra_bn_workspace_floats(C)))
    return rc;
  hipStream_t st = as_stream(stream);
  const float inv_n = 1.f / (float)npix;
  const int form = bn_form(RA_BN_PASS_MOMENTS, C, npix, 0, 1, 0, 3, 0);
  if (form == RA_BN_FORM_SMALL) {
    hipLaunchKernelGGL(train::moments_small_kernel, dim3(1), dim3(train::kSmallThreads), 0, st, u, npix * C, C, inv_n, mean, var);
    return launch_status(who);
  }
  // two passes of nb partial blocks and a finish each: the sums about nothing give the mean, the squares about the mean the variance
  const int C4 = C / 4, n4 = (int)(npix * C4);
  const size_t lanes = 256 / C, want = form == RA_BN_FORM_V4 ? (size_t)ceil_div(n4, 256) : (npix + lanes - 1) / lanes;
  const int nb = want < (size_t)kRedBlocks ? (int)want : kRedBlocks;
  for (int pass = 0; pass < 2; ++pass) {
    const float *about = pass ? mean : nullptr;
    if (form == RA_BN_FORM_V4)
      hipLaunchKernelGGL(train::chan_sum_v4_kernel, dim3(nb), dim3(256), 0, st, reinterpret_cast<const train::f32x4 *>(u), n4, C4, about, ws);
    else
      hipLaunchKernelGGL(train::chan_sum_kernel, dim3(nb), dim3(256), 0, st, u, npix, C, about, ws);
    hipLaunchKernelGGL(train::chan_final_kernel, dim3(C), dim3(256), 0, st, ws, nb, C, inv_n, pass ? var : mean);
  }
  return launch_status(who);
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

// flags: bit 0 = u is stored as bf16, bit 1 = y is written as bf16 (only combinations the bf16 mode produces: 0, 1, 3)
extern "C" int ra_bn_act_pool_bf16_f32(const void *u, const float *mean, const float *var, const float *gamma, const float *beta,
                                       float eps, int relu, int pool, int B, int H, int W, int C, void *y, int flags, void *stream) {
  const char *who = flags ? "ra_bn_act_pool_bf16_f32" : "ra_bn_act_pool_f32";
  if (const int rc = check_call(who, u && y && B > 0 && H > 0 && W > 0, C, 0x7fffffff, pool, H, W, 0, 0)) return rc;
  hipStream_t st = as_stream(stream);
  const int form = bn_form(RA_BN_PASS_FORWARD, C, (size_t)B * H * W, W, pool, flags, 3, 0);
  if (form < 0) return form_error(form, who, C, flags);
  if (form == RA_BN_FORM_V4) {
    const V4Grid g(C, B, H, W, pool);
    with_storage(pool, flags, [&](auto P, auto UB, auto YB) {
      typedef train::Q4<decltype(UB)::value> QU;
      typedef train::Q4<decltype(YB)::value> QY;
      hipLaunchKernelGGL((train::bn_act_pool_v4_kernel<decltype(P)::value, decltype(UB)::value, decltype(YB)::value>), g.elementwise(),
                         dim3(256), 0, st, reinterpret_cast<const typename QU::T *>(u), mean, var, gamma, beta, eps, relu, B, H, W, g.C4,
                         g.lg, reinterpret_cast<typename QY::T *>(y));
    });
    return launch_status(who);
  }
  const size_t total = (size_t)B * (H / pool) * (W / pool) * C;
  size_t grid = (total + 255) / 256;
  if (grid > 8192) grid = 8192;
  hipLaunchKernelGGL(train::bn_act_pool_kernel, dim3((unsigned)grid), dim3(256), 0, st, static_cast<const float *>(u), mean, var, gamma,
                     beta, eps, relu, pool, B, H, W, C, static_cast<float *>(y));
  return launch_status(who);
}

extern "C" int ra_bn_act_pool_f32(const float *u, const float *mean, const float *var, const float *gamma,
                                  const float *beta, float eps, int relu, int pool, int B, int H, int W, int C, float *y,
                                  void *stream) {
  return ra_bn_act_pool_bf16_f32(u, mean, var, gamma, beta, eps, relu, pool, B, H, W, C, y, 0, stream);
}

namespace {
// One BatchNorm backward call, or (tabs != nullptr) G calls of one layer — its G timesteps — stacked along the batch: u
// [G*B,H,W,C], dy [G*B,H/pool,W/pool,C], one reduce / final / dx triple in which every group has its own statistics and
// parameters, read through a device table of 6 G pointers {mean, var, gamma, beta, grad-bucket gamma, grad-bucket beta}[G];
// dgamma / dbeta [G,C].
// stages: 1 = the two reductions (dbeta, dgamma over THIS call's pixels), 2 = du from dbeta / dgamma and the count
// they were summed over (n_total; 0 = this call's B*H*W).  Data-parallel training with whole-batch statistics
// runs stage 1, all-reduces the 2C sums, then stage 2 with the global count (ra_train.ConvBNActPool).
// flags (the bf16 mode, model_opt['compute_dtype'] = 'bf16'): bit 0 = u is read and du written as bf16, bit 1 = dy is read as
// bf16 (0, 1 or 3); float32 statistics, sums and parameter gradients.
int bn_bwd_impl(const void *u, const void *dy, const float *mean, const float *var, const float *gamma, const float *beta,
                const void *const *tabs, int G, bool grouped, float eps, int relu, int pool, int B, int H, int W, int C, float *ws,
                size_t ws_floats, float *dgamma, float *dbeta, void *du, float *acc_gamma, float *acc_beta, void *stream,
                int stages = 3, double n_total = 0.0, int flags = 0) {
  const char *who = grouped ? "ra_bn_act_pool_bwd_grouped_f32" : "ra_bn_act_pool_bwd_f32";
  const bool ok = u && dy && dgamma && dbeta && (!(stages & 1) || ws) && (!(stages & 2) || du) && (!grouped || (tabs && G > 0)) &&
                  B > 0 && H > 0 && W > 0;
  const size_t ws_need = grouped ? (size_t)G * ra_bn_workspace_floats(C) : (stages & 1) ? ra_bn_workspace_floats(C) : 0;
  if (const int rc = check_call(who, ok, C, grouped ? 0x7fffffff : train::kMaxC, pool, H, W, ws_floats, ws_need)) return rc;
  hipStream_t st = as_stream(stream);
  const size_t npix = (size_t)B * H * W;
  const float inv_n = (float)(1.0 / (n_total > 0.0 ? n_total : (double)npix));
  const float *const *ct = reinterpret_cast<const float *const *>(tabs);
  const int Gz = grouped ? G : 1;
  const int form = bn_form(RA_BN_PASS_BACKWARD, C, npix, W, pool, flags, stages, grouped ? G : 0);
  if (form < 0) return form_error(form, who, C, flags);
  if (form == RA_BN_FORM_V4) {
    const V4Grid g(C, B, H, W, pool);
    float *const *mt = reinterpret_cast<float *const *>(const_cast<void *const *>(tabs));
    with_storage(pool, flags, [&](auto P, auto UB, auto DB) {
      constexpr int POOL = decltype(P)::value;
      constexpr bool ub = decltype(UB)::value, db = decltype(DB)::value;
      typedef typename train::Q4<ub>::T TU;
      typedef typename train::Q4<db>::T TD;
      const TU *u4 = reinterpret_cast<const TU *>(u);
      const TD *dy4 = reinterpret_cast<const TD *>(dy);
      if (stages & 1) {
        hipLaunchKernelGGL((train::bn_bwd_reduce_v4_kernel<POOL, ub, db>), g.reduce(Gz), dim3(256), 0, st, u4, dy4, mean, var, gamma, beta,
                           eps, relu, B, H, W, g.C4, g.lg, ws, ct, Gz);
        hipLaunchKernelGGL(train::bn_bwd_final_kernel, dim3(C, Gz), dim3(256), 0, st, ws, g.partials(), C, dbeta, dgamma, acc_beta,
                           acc_gamma, mt, Gz);
      }
      if (stages & 2)
        hipLaunchKernelGGL((train::bn_bwd_dx_v4_kernel<POOL, ub, db>), g.elementwise(Gz), dim3(256), 0, st, u4, dy4, mean, var, gamma, beta,
                           dbeta, dgamma, eps, relu, B, H, W, g.C4, g.lg, reinterpret_cast<TU *>(du), inv_n, ct, Gz);
    });
    return launch_status(who);
  }
  const float *uf = static_cast<const float *>(u), *dyf = static_cast<const float *>(dy);
  float *duf = static_cast<float *>(du);
  if (form == RA_BN_FORM_SMALL) {  // one workgroup per call or group
    hipLaunchKernelGGL(train::bn_bwd_small_kernel, dim3(Gz), dim3(train::kSmallThreads), 0, st, uf, dyf, mean, var, gamma, beta, eps, relu,
                       pool, B, H, W, C, dbeta, dgamma, acc_beta, acc_gamma, duf, inv_n, ct, Gz);
    return launch_status(who);
  }
  const size_t lanes = 256 / C, nbl = (npix + lanes - 1) / lanes;
  const int nb = nbl < (size_t)kRedBlocks ? (int)nbl : kRedBlocks;
  if (stages & 1) {
    hipLaunchKernelGGL(train::bn_bwd_reduce_kernel, dim3(nb), dim3(256), 0, st, uf, dyf, mean, var, gamma, beta, eps, relu, pool,
                       B, H, W, C, ws);
    hipLaunchKernelGGL(train::bn_bwd_final_kernel, dim3(C), dim3(256), 0, st, ws, nb, C, dbeta, dgamma, acc_beta, acc_gamma);
  }
  if (stages & 2) {
    size_t grid = (npix * C + 255) / 256;
    if (grid > 8192) grid = 8192;
    hipLaunchKernelGGL(train::bn_bwd_dx_kernel, dim3((unsigned)grid), dim3(256), 0, st, uf, dyf, mean, var, gamma, beta, dbeta,
                       dgamma, eps, relu, pool, B, H, W, C, duf, inv_n);
  }
  return launch_status(who);
}
}  // namespace

extern "C" int ra_bn_act_pool_bwd_grouped_bf16_f32(const void *u, const void *dy, const void *const *tabs, int G, float eps, int relu,
                                                   int pool, int B, int H, int W, int C, float *ws, size_t ws_floats, float *dgamma,
                                                   float *dbeta, void *du, int flags, void *stream) {
  return bn_bwd_impl(u, dy, nullptr, nullptr, nullptr, nullptr, tabs, G, true, eps, relu, pool, B, H, W, C, ws, ws_floats, dgamma, dbeta,
                     du, nullptr, nullptr, stream, 3, 0.0, flags);
}

extern "C" int ra_bn_act_pool_bwd_grouped_f32(const float *u, const float *dy, const void *const *tabs, int G, float eps, int relu,
                                              int pool, int B, int H, int W, int C, float *ws, size_t ws_floats, float *dgamma,
                                              float *dbeta, float *du, void *stream) {
  return ra_bn_act_pool_bwd_grouped_bf16_f32(u, dy, tabs, G, eps, relu, pool, B, H, W, C, ws, ws_floats, dgamma, dbeta, du, 0, stream);
}

extern "C" int ra_bn_act_pool_bwd_acc_bf16_f32(const void *u, const void *dy, const float *mean, const float *var, const float *gamma,
                                               const float *beta, float eps, int relu, int pool, int B, int H, int W, int C, float *ws,
                                               size_t ws_floats, float *dgamma, float *dbeta, void *du, float *acc_gamma,
                                               float *acc_beta, int flags, void *stream) {
  return bn_bwd_impl(u, dy, mean, var, gamma, beta, nullptr, 1, false, eps, relu, pool, B, H, W, C, ws, ws_floats, dgamma, dbeta, du,
                     acc_gamma, acc_beta, stream, 3, 0.0, flags);
}

extern "C" int ra_bn_act_pool_bwd_acc_f32(const float *u, const float *dy, const float *mean, const float *var,
                                          const float *gamma, const float *beta, float eps, int relu, int pool, int B,
                                          int H, int W, int C, float *ws, size_t ws_floats, float *dgamma, float *dbeta,
                                          float *du, float *acc_gamma, float *acc_beta, void *stream) {
  return bn_bwd_impl(u, dy, mean, var, gamma, beta, nullptr, 1, false, eps, relu, pool, B, H, W, C, ws, ws_floats, dgamma, dbeta, du,
                     acc_gamma, acc_beta, stream);
}

extern "C" int ra_bn_act_pool_bwd_f32(const float *u, const float *dy, const float *mean, const float *var,
                                      const float *gamma, const float *beta, float eps, int relu, int pool, int B,
                                      int H, int W, int C, float *ws, size_t ws_floats, float *dgamma, float *dbeta,
                                      float *du, void *stream) {
  return ra_bn_act_pool_bwd_acc_f32(u, dy, mean, var, gamma, beta, eps, relu, pool, B, H, W, C, ws, ws_floats, dgamma, dbeta, du,
                                    nullptr, nullptr, stream);
}

extern "C" int ra_bn_act_pool_bwd_reduce_f32(const float *u, const float *dy, const float *mean, const float *var,
                                             const float *gamma, const float *beta, float eps, int relu, int pool, int B,
                                             int H, int W, int C, float *ws, size_t ws_floats, float *dgamma, float *dbeta,
                                             float *acc_gamma, float *acc_beta, void *stream) {
  return bn_bwd_impl(u, dy, mean, var, gamma, beta, nullptr, 1, false, eps, relu, pool, B, H, W, C, ws, ws_floats, dgamma, dbeta,
                     nullptr, acc_gamma, acc_beta, stream, 1);
}

extern "C" int ra_bn_act_pool_bwd_dx_f32(const float *u, const float *dy, const float *mean, const float *var,
                                         const float *gamma, const float *beta, const float *dgamma_sum,
                                         const float *dbeta_sum, double n_total, float eps, int relu, int pool, int B, int H,
                                         int W, int C, float *du, void *stream) {
  return bn_bwd_impl(u, dy, mean, var, gamma, beta, nullptr, 1, false, eps, relu, pool, B, H, W, C, nullptr, 0,
                     const_cast<float *>(dgamma_sum), const_cast<float *>(dbeta_sum), du, nullptr, nullptr, stream, 2, n_total);
}
