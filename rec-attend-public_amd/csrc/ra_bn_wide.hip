// Train-mode BatchNorm for the wide layers of fg_model (nnlib.py:98-119,250-253; fg_model.py:112-160 with 192 .. 512 channels):
// ra_bn.hip's three passes with its arithmetic — biased variance taken about the mean in a second pass, eps inside the square
// root, the pool's gradient to the first maximum of a window, the statistics differentiated through — for ANY C % 4 == 0 up to 512.
// ra_bn.hip's float4 kernels need C / 4 to be a power of two (192 and 512 are out: its moments stop at 256) and its scalar
// ones moved 0.5 TB/s.  Here a workgroup is PL x C / 4 threads, PL = 256 / (C / 4) (the rest idle): a thread owns one channel
// quad of one pooling window (float4 loads) and walks the windows PL gridDim apart, so its quad never changes.
// Reductions are two-stage and fixed-order, no atomics: a workgroup adds its PL lanes in LDS in lane order and leaves one record;
// the finishing launch gives a channel one wave, which strides over the (at most kWideBlocks) records and ends in a fixed butterfly.
#include <type_traits>

#include "ra_bn_parts.h"

namespace ra {
namespace train {

constexpr int kWideBlocks = 256;  // records per channel that a reduction leaves
constexpr int kWideMaxC = 512;

struct WideThread {
  int pl, cg, PL;
  bool live;
  __device__ WideThread(int C4) : pl(threadIdx.x / C4), cg(threadIdx.x % C4), PL(256 / C4), live(pl < PL) {}
};

// the sum of v over the lanes of a workgroup that share a channel quad, lane order; valid in threads tid < C4
__device__ inline f32x4 sum_lanes(f32x4 v, int C4, int PL, f32x4 *red) {
  __syncthreads();
  red[threadIdx.x] = v;
  __syncthreads();
  f32x4 t = f32x4{0.f, 0.f, 0.f, 0.f};
  if ((int)threadIdx.x < C4) {
    t = red[threadIdx.x];
    for (int l = 1; l < PL; ++l) t += red[l * C4 + threadIdx.x];
  }
  return t;
}

// per-channel sum (mean == nullptr) or sum of squared deviations over u [npix][C4] float4s -> part [gridDim.x][C]
__global__ __launch_bounds__(256) void wide_chan_sum_kernel(const f32x4 *u, size_t npix, int C4, const float *mean, f32x4 *part) {
  __shared__ f32x4 red[256];
  const WideThread t(C4);
  f32x4 mu = f32x4{0.f, 0.f, 0.f, 0.f}, s = mu;
  if (t.live) {
    if (mean)
      for (int i = 0; i < 4; ++i) mu[i] = mean[4 * t.cg + i];
    for (size_t p = (size_t)blockIdx.x * t.PL + t.pl; p < npix; p += (size_t)gridDim.x * t.PL) {
      const f32x4 v = u[p * C4 + t.cg] - mu;
      s += mean ? v * v : v;
    }
  }
  const f32x4 tot = sum_lanes(s, C4, t.PL, red);
  if ((int)threadIdx.x < C4) part[(size_t)blockIdx.x * C4 + threadIdx.x] = tot;
}

// one wave per channel: NV vectors of records part [nblocks][NV][C] -> their sums, lane-strided then a fixed butterfly
template <int NV>
__device__ inline void wave_record_sums(const float *part, int nblocks, int C, int c, float (&t)[NV]) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int v = 0; v < NV; ++v) t[v] = 0.f;
  for (int k = lane; k < nblocks; k += 64)
#pragma unroll
    for (int v = 0; v < NV; ++v) t[v] += part[((size_t)k * NV + v) * C + c];
#pragma unroll
  for (int v = 0; v < NV; ++v)
    for (int o = 32; o > 0; o >>= 1) t[v] += __shfl_xor(t[v], o, 64);
}

__global__ __launch_bounds__(256) void wide_chan_final_kernel(const float *part, int nblocks, int C, float inv_n, float *out) {
  const int c = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= C) return;
  float t[1];
  wave_record_sums<1>(part, nblocks, C, c, t);
  if ((threadIdx.x & 63) == 0) out[c] = t[0] * inv_n;
}

// window wi of [B][Ho][Wo] -> its first pixel's float4 index in u (without the channel quad)
struct WideWindow {
  size_t first;
  int W;
  __device__ WideWindow(size_t wi, int Ho, int Wo, int H, int W_, int POOL) : W(W_) {
    const int xo = (int)(wi % Wo);
    const size_t r = wi / Wo;
    const int yo = (int)(r % Ho);
    const size_t b = r / Ho;
    first = (b * H + (size_t)yo * POOL) * W_ + (size_t)xo * POOL;
  }
  __device__ size_t pixel(int q, int POOL) const { return first + (size_t)(q / POOL) * W + (q % POOL); }
};

template <int POOL>
__global__ __launch_bounds__(256) void wide_act_pool_kernel(const f32x4 *u, const float *mean, const float *var, const float *gamma,
                                                            const float *beta, float eps, int relu, size_t nwin, int H, int W, int C4,
                                                            f32x4 *y) {
  const WideThread t(C4);
  if (!t.live) return;
  const int Ho = H / POOL, Wo = W / POOL;
  const BnConst k = bn_const(mean, var, gamma, beta, eps, 4 * t.cg);
  const float lo = relu ? 0.f : -__builtin_inff();
  for (size_t wi = (size_t)blockIdx.x * t.PL + t.pl; wi < nwin; wi += (size_t)gridDim.x * t.PL) {
    const WideWindow win(wi, Ho, Wo, H, W, POOL);
    f32x4 w[POOL * POOL], best;
#pragma unroll
    for (int q = 0; q < POOL * POOL; ++q) w[q] = u[win.pixel(q, POOL) * C4 + t.cg];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float m = -__builtin_inff();
#pragma unroll
      for (int q = 0; q < POOL * POOL; ++q) m = fmaxf(m, fmaxf((w[q][i] - k.mu[i]) * k.g[i] + k.be[i], lo));
      best[i] = m;
    }
    y[wi * C4 + t.cg] = best;
  }
}

// stage 1: part [gridDim.x][2][C] = this workgroup's sums of dv and of dv * xhat
template <int POOL>
__global__ __launch_bounds__(256) void wide_bwd_reduce_kernel(const f32x4 *u, const f32x4 *dy, const float *mean, const float *var,
                                                              const float *gamma, const float *beta, float eps, int relu, size_t nwin,
                                                              int H, int W, int C4, f32x4 *part) {
  __shared__ f32x4 red[256];
  const WideThread t(C4);
  const int Ho = H / POOL, Wo = W / POOL;
  f32x4 s0 = f32x4{0.f, 0.f, 0.f, 0.f}, s1 = s0;
  if (t.live) {
    const BnConst k = bn_const(mean, var, gamma, beta, eps, 4 * t.cg);
    const float lo = relu ? 0.f : -__builtin_inff();
    for (size_t wi = (size_t)blockIdx.x * t.PL + t.pl; wi < nwin; wi += (size_t)gridDim.x * t.PL) {
      const WideWindow win(wi, Ho, Wo, H, W, POOL);
      f32x4 w[POOL * POOL], dv[POOL * POOL], xh[POOL * POOL];
#pragma unroll
      for (int q = 0; q < POOL * POOL; ++q) w[q] = u[win.pixel(q, POOL) * C4 + t.cg];
      window_grad<POOL>(w, dy[wi * C4 + t.cg], k, lo, relu, dv, xh);
#pragma unroll
      for (int q = 0; q < POOL * POOL; ++q) {
        s0 += dv[q];
        s1 += dv[q] * xh[q];
      }
    }
  }
  const f32x4 t0 = sum_lanes(s0, C4, t.PL, red), t1 = sum_lanes(s1, C4, t.PL, red);
  if ((int)threadIdx.x < C4) {
    part[((size_t)blockIdx.x * 2) * C4 + threadIdx.x] = t0;
    part[((size_t)blockIdx.x * 2 + 1) * C4 + threadIdx.x] = t1;
  }
}

__global__ __launch_bounds__(256) void wide_bwd_final_kernel(const float *part, int nblocks, int C, float *dbeta, float *dgamma,
                                                             float *acc_beta, float *acc_gamma) {
  const int c = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= C) return;
  float t[2];
  wave_record_sums<2>(part, nblocks, C, c, t);
  if ((threadIdx.x & 63) == 0) {
    dbeta[c] = t[0];
    dgamma[c] = t[1];
    if (acc_beta) acc_beta[c] += t[0];  // straight into the gradient bucket (one writer per element)
    if (acc_gamma) acc_gamma[c] += t[1];
  }
}

// stage 2: du = gamma rstd (dv - dbeta / n - xhat dgamma / n), or du = dv without BatchNorm (var == nullptr)
template <int POOL>
__global__ __launch_bounds__(256) void wide_bwd_dx_kernel(const f32x4 *u, const f32x4 *dy, const float *mean, const float *var,
                                                          const float *gamma, const float *beta, const float *dbeta, const float *dgamma,
                                                          float eps, int relu, size_t nwin, int H, int W, int C4, float inv_n, f32x4 *du) {
  const WideThread t(C4);
  if (!t.live) return;
  const int Ho = H / POOL, Wo = W / POOL;
  const BnConst k = bn_const(mean, var, gamma, beta, eps, 4 * t.cg);
  const float lo = relu ? 0.f : -__builtin_inff();
  f32x4 db, dg;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    db[i] = dbeta[4 * t.cg + i] * inv_n;
    dg[i] = dgamma[4 * t.cg + i] * inv_n;
  }
  for (size_t wi = (size_t)blockIdx.x * t.PL + t.pl; wi < nwin; wi += (size_t)gridDim.x * t.PL) {
    const WideWindow win(wi, Ho, Wo, H, W, POOL);
    f32x4 w[POOL * POOL], dv[POOL * POOL], xh[POOL * POOL];
#pragma unroll
    for (int q = 0; q < POOL * POOL; ++q) w[q] = u[win.pixel(q, POOL) * C4 + t.cg];
    window_grad<POOL>(w, dy[wi * C4 + t.cg], k, lo, relu, dv, xh);
#pragma unroll
    for (int q = 0; q < POOL * POOL; ++q) du[win.pixel(q, POOL) * C4 + t.cg] = var ? k.g * (dv[q] - db - xh[q] * dg) : dv[q];
  }
}

}  // namespace train
}  // namespace ra

using namespace ra;

namespace {
int wide_check(const char *who, bool args_ok, int C, int pool, int H, int W, size_t ws_have, size_t ws_need) {
  if (!args_ok || C <= 0) return fail(RA_E_INVALID, "%s: bad argument", who);
  if (C % 4 || C > train::kWideMaxC) return fail(RA_E_SHAPE, "%s: C %d (%% 4, <= %d)", who, C, train::kWideMaxC);
  if ((pool != 1 && pool != 2) || (pool == 2 && ((H | W) & 1))) return fail(RA_E_SHAPE, "%s: pool", who);
  if (ws_have < ws_need) return fail(RA_E_WORKSPACE, "%s: workspace too small", who);
  return 0;
}
// workgroups of a pass over n windows, PL of them per workgroup and round
int wide_blocks(size_t n, int C, int most) {
  const size_t PL = 256 / (C / 4), want = (n + PL - 1) / PL;
  return want < (size_t)most ? (int)want : most;
}
}  // namespace

extern "C" size_t ra_bn_wide_workspace_floats(int C) { return (size_t)train::kWideBlocks * 2 * (C > 0 ? C : 1); }

extern "C" int ra_bn_wide_moments_f32(const float *u, size_t npix, int C, float *ws, size_t ws_floats, float *mean, float *var,
                                      void *stream) {
  const char *who = "ra_bn_wide_moments_f32";
  if (const int rc = wide_check(who, u && ws && mean && var && npix != 0, C, 1, 0, 0, ws_floats, ra_bn_wide_workspace_floats(C))) return rc;
  hipStream_t st = as_stream(stream);
  const float inv_n = 1.f / (float)npix;
  const int nb = wide_blocks(npix, C, train::kWideBlocks);
  // two passes of nb records and a finish each: the sums about nothing give the mean, the squares about the mean the variance
  for (int pass = 0; pass < 2; ++pass) {
    hipLaunchKernelGGL(train::wide_chan_sum_kernel, dim3(nb), dim3(256), 0, st, reinterpret_cast<const train::f32x4 *>(u), npix, C / 4,
                       pass ? mean : nullptr, reinterpret_cast<train::f32x4 *>(ws));
    hipLaunchKernelGGL(train::wide_chan_final_kernel, dim3(ceil_div(C, 4)), dim3(256), 0, st, ws, nb, C, inv_n, pass ? var : mean);
  }
  return launch_status(who);
}

extern "C" int ra_bn_wide_act_pool_f32(const float *u, const float *mean, const float *var, const float *gamma, const float *beta,
                                       float eps, int relu, int pool, int B, int H, int W, int C, float *y, void *stream) {
  const char *who = "ra_bn_wide_act_pool_f32";
  if (const int rc = wide_check(who, u && y && B > 0 && H > 0 && W > 0, C, pool, H, W, 0, 0)) return rc;
  const size_t nwin = (size_t)B * (H / pool) * (W / pool);
  const int nb = wide_blocks(nwin, C, 16384);
  typedef train::f32x4 V;
  if (pool == 2)
    hipLaunchKernelGGL(train::wide_act_pool_kernel<2>, dim3(nb), dim3(256), 0, as_stream(stream), (const V *)u, mean, var, gamma, beta, eps,
                       relu, nwin, H, W, C / 4, (V *)y);
  else
    hipLaunchKernelGGL(train::wide_act_pool_kernel<1>, dim3(nb), dim3(256), 0, as_stream(stream), (const V *)u, mean, var, gamma, beta, eps,
                       relu, nwin, H, W, C / 4, (V *)y);
  return launch_status(who);
}

extern "C" int ra_bn_wide_act_pool_bwd_acc_f32(const float *u, const float *dy, const float *mean, const float *var, const float *gamma,
                                               const float *beta, float eps, int relu, int pool, int B, int H, int W, int C, float *ws,
                                               size_t ws_floats, float *dgamma, float *dbeta, float *du, float *acc_gamma,
                                               float *acc_beta, void *stream) {
  const char *who = "ra_bn_wide_act_pool_bwd_acc_f32";
  if (const int rc = wide_check(who, u && dy && ws && dgamma && dbeta && du && B > 0 && H > 0 && W > 0, C, pool, H, W, ws_floats,
                                ra_bn_wide_workspace_floats(C)))
    return rc;
  hipStream_t st = as_stream(stream);
  const size_t nwin = (size_t)B * (H / pool) * (W / pool);
  const int nr = wide_blocks(nwin, C, train::kWideBlocks), nx = wide_blocks(nwin, C, 16384), C4 = C / 4;
  const float inv_n = 1.f / (float)((size_t)B * H * W);
  typedef train::f32x4 V;
  auto run = [&](auto P) {
    constexpr int POOL = decltype(P)::value;
    hipLaunchKernelGGL(train::wide_bwd_reduce_kernel<POOL>, dim3(nr), dim3(256), 0, st, (const V *)u, (const V *)dy, mean, var, gamma, beta, eps,
                       relu, nwin, H, W, C4, (V *)ws);
    hipLaunchKernelGGL(train::wide_bwd_final_kernel, dim3(ceil_div(C, 4)), dim3(256), 0, st, ws, nr, C, dbeta, dgamma, acc_beta, acc_gamma);
    hipLaunchKernelGGL(train::wide_bwd_dx_kernel<POOL>, dim3(nx), dim3(256), 0, st, (const V *)u, (const V *)dy, mean, var, gamma, beta, dbeta,
                       dgamma, eps, relu, nwin, H, W, C4, inv_n, (V *)du);
  };
  if (pool == 2) run(std::integral_constant<int, 2>{});
  else run(std::integral_constant<int, 1>{});
  return launch_status(who);
}
