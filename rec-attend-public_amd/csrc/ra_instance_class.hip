// K14 — the Cityscapes output stage behind the decode loop: which semantic class an instance is, and the foreground
// mask of the pre-stage's semantic map (cityscapes_eval.py:148-205, analysis.py:196-267 RenderCityScapesOutputAnalyzer).
//
//   sem_foreground   cityscapes_eval.py:166-176: channel 0 (C == 1: the only channel) of the semantic map resized to the
//                    labels' size with cv2.resize(..., INTER_LINEAR) and compared with FG_THRESHOLD, fused: the full-size
//                    map is never written.
//   vote             analysis.py:235-237: vote[b,t,c] = mean over the H x W pixels of y[b,t] * sem_h[b,...,c], a skinny
//                    [T x HW] . [HW x C] product whose right operand is the resized semantic map.  It is evaluated on the
//                    fly, 256 pixels at a time into LDS (four taps per channel out of the small map, which stays in L2), so
//                    the C full-size planes are never materialised; y is read exactly once, 16 bytes per lane.
//   pick             analysis.py:251-261: conf > 0.5 and vote[0] <= 0.7 -> arg-max of vote[1:] (first maximum), else -1.
//
// The resize restates cv2's float path: source coordinate (d + 0.5) * (src / dst) - 0.5 evaluated in double, the fraction
// rounded to float once, taps clamped to the image, rows interpolated along W first and then along H, all in float32.
// Double for the coordinate because cv2 does so and because a float coordinate is a few 1e-6 off at non-integer ratios
// (48 -> 100: one ulp of 47 is 3.8e-6), which an edge of the map turns into a value error above the 2e-6 the decisions
// built on it are held to; ra_resize_linear_f32 (ra_eval.hip) keeps its float coordinate, exact at integer ratios.
#include <cmath>
#include <cstdint>

#include "ra_common.h"
#include "ra_gt_ids.h"
#include "ra_resample.h"

namespace ra {
namespace icls {

typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr int kMaxT = 32;               // the evaluator's limit (ra_eval.hip)
constexpr int kMaxC = 16;
constexpr int kTile = 256;              // pixels per tile = threads per workgroup
constexpr int kWaves = kTile / kWave;   // 4
constexpr int kTPerWave = kMaxT / kWaves;  // a wave owns the instances wave, wave + 4, ...: at most 8 (KT below: 5 up to T = 20)
constexpr int kTargetWgs = 1024;        // four workgroups per CU: what the 127 registers of vote_kernel<9, 5> leave room for

using resample::tap;  // one axis of the resize: the two taps and the fraction, coordinate in double

// One thread per output pixel.
__global__ __launch_bounds__(256) void sem_foreground_kernel(const float *sem, int Hs, int Ws, int C, int H, int W,
                                                              double sy, double sx, float thresh, float lim, float *fg) {
  const int b = blockIdx.y;
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= H * W) return;
  const int r = e / W, c = e - r * W;
  int y0, y1, x0, x1;
  float fy, fx;
  tap(r, Hs, sy, y0, y1, fy);
  tap(c, Ws, sx, x0, x1, fx);
  const float *p = sem + (size_t)b * Hs * Ws * C;
  const float top = p[((size_t)y0 * Ws + x0) * C] * (1.f - fx) + p[((size_t)y0 * Ws + x1) * C] * fx;
  const float bot = p[((size_t)y1 * Ws + x0) * C] * (1.f - fx) + p[((size_t)y1 * Ws + x1) * C] * fx;
  const float v = top * (1.f - fy) + bot * fy;
  // cityscapes_eval.py:172-176: one channel = a foreground map, several = channel 0 is the background.  Both compare a
  // float32 array with a Python float, which numpy does in float32 (the scalar is rounded to the array's type): float here too
  fg[(size_t)b * H * W + e] = (C == 1 ? v > thresh : v <= lim) ? 1.f : 0.f;
}

// Workgroup (x, b) walks the tiles x, x + gridDim.x, ... of image b.  Per tile: every thread issues its y loads, resizes one
// pixel of the semantic map for all C channels into LDS ([c][pixel]), and after the barrier wave w multiplies the
// instances w, w + 4, ... (their 4 pixels per lane) with the tile's C x 256 values.  Accumulators stay in registers over
// the whole walk; one wave reduction per (t, c) at the end, written to part[b][t][c][x] — no atomics, and the finishing
// launch adds the workgroups in a fixed order, so the result does not depend on the order they ran in.  KT = the instances
// a wave can own (its accumulators are KT x C registers: 5 for T <= 20, Cityscapes' 20 among them, else 8).
template <int C, int KT>
__global__ __launch_bounds__(256) void vote_kernel(const float *y, const float *sem, int T, int HW, int W, int Hs, int Ws,
                                                    double sy, double sx, int ntiles, int vec_ok, float *part) {
  __shared__ __attribute__((aligned(16))) float sh[C][kTile];  // read back 16 bytes at a time
  const int b = blockIdx.y, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int nk = wave < T ? (T - wave + kWaves - 1) / kWaves : 0;  // instances of this wave (uniform)
  const float *semb = sem + (size_t)b * Hs * Ws * C;
  const float *yb = y + (size_t)b * T * HW;
  float acc[KT][C];
#pragma unroll
  for (int k = 0; k < KT; ++k)
#pragma unroll
    for (int ch = 0; ch < C; ++ch) acc[k][ch] = 0.f;

  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    // (1) this lane's 4 pixels of every instance the wave owns: the only read of y
    const int base = tile * kTile + 4 * lane;
    f32x4 v[KT];
#pragma unroll
    for (int k = 0; k < KT; ++k) {
      v[k] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (k < nk) {
        const float *q = yb + (size_t)(wave + kWaves * k) * HW + base;
        if (vec_ok) {  // H * W % 4 == 0 and 16-byte aligned: base < HW implies base + 3 < HW
          if (base < HW) v[k] = __builtin_nontemporal_load(reinterpret_cast<const f32x4 *>(q));
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (base + j < HW) v[k][j] = q[j];
        }
      }
    }
    // (2) the semantic map at this thread's pixel, all channels
    const int p = tile * kTile + tid;
    if (p < HW) {
      const int r = p / W, c = p - r * W;
      int y0, y1, x0, x1;
      float fy, fx;
      tap(r, Hs, sy, y0, y1, fy);
      tap(c, Ws, sx, x0, x1, fx);
      const float *p00 = semb + ((size_t)y0 * Ws + x0) * C, *p01 = semb + ((size_t)y0 * Ws + x1) * C;
      const float *p10 = semb + ((size_t)y1 * Ws + x0) * C, *p11 = semb + ((size_t)y1 * Ws + x1) * C;
#pragma unroll
      for (int ch = 0; ch < C; ++ch) {
        const float top = p00[ch] * (1.f - fx) + p01[ch] * fx;
        const float bot = p10[ch] * (1.f - fx) + p11[ch] * fx;
        sh[ch][tid] = top * (1.f - fy) + bot * fy;
      }
    } else {
#pragma unroll
      for (int ch = 0; ch < C; ++ch) sh[ch][tid] = 0.f;
    }
    __syncthreads();
    // (3) [nk x 4] . [4 x C] per lane (a wave's unused v[k] are zero)
#pragma unroll
    for (int ch = 0; ch < C; ++ch) {
      const f32x4 s = *reinterpret_cast<const f32x4 *>(&sh[ch][4 * lane]);
#pragma unroll
      for (int k = 0; k < KT; ++k) acc[k][ch] += v[k][0] * s[0] + v[k][1] * s[1] + v[k][2] * s[2] + v[k][3] * s[3];
    }
    __syncthreads();
  }

  float *o = part + (size_t)b * T * C * gridDim.x + blockIdx.x;
#pragma unroll
  for (int k = 0; k < KT; ++k)
    if (k < nk) {
#pragma unroll
      for (int ch = 0; ch < C; ++ch) {
        float a = acc[k][ch];
        for (int off = 32; off > 0; off >>= 1) a += __shfl_xor(a, off, 64);
        if (lane == 0) o[(size_t)((wave + kWaves * k) * C + ch) * gridDim.x] = a;
      }
    }
}

__device__ __forceinline__ void pick_one(const float *vote, float conf, int C, int *class_idx, int *label_id) {
  int idx = -1;
  if (conf > 0.5f && (double)vote[0] <= 0.7) {  // analysis.py:232,251
    idx = 0;
    float best = vote[1];
    for (int c = 2; c < C; ++c)
      if (vote[c] > best) {  // strict: the first maximum, like numpy.argmax
        best = vote[c];
        idx = c - 1;
      }
  }
  if (class_idx) *class_idx = idx;
  if (label_id) *label_id = idx >= 0 && idx < gtid::kCsClasses ? gtid::cs_label_id(idx) : -1;
}

// One workgroup per instance (b, t): wave w adds the nwg partials of the channels w, w + 4, ... — lane l takes the workgroups
// l, l + 64, ... in that order, then a butterfly over the lanes, all in double: a fixed order — takes the mean, and
// thread 0 picks.
__global__ __launch_bounds__(256) void vote_finish_kernel(const float *part, int nwg, int T, int C, double inv_hw,
                                                           const float *conf, float *vote, int *class_idx, int *label_id) {
  __shared__ float sv[kMaxC];
  const int t = blockIdx.x, b = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const size_t inst = (size_t)b * T + t;
  for (int ch = wave; ch < C; ch += kWaves) {
    const float *p = part + (inst * C + ch) * nwg;
    double s = 0.0;
    for (int w = lane; w < nwg; w += kWave) s += (double)p[w];
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if (lane == 0) {
      const float m = (float)(s * inv_hw);
      vote[inst * C + ch] = m;
      sv[ch] = m;
    }
  }
  __syncthreads();
  if (conf && threadIdx.x == 0)
    pick_one(sv, conf[inst], C, class_idx ? class_idx + inst : nullptr, label_id ? label_id + inst : nullptr);
}

__global__ __launch_bounds__(256) void pick_kernel(const float *vote, const float *conf, int N, int C, int *class_idx,
                                                    int *label_id) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  pick_one(vote + (size_t)i * C, conf[i], C, class_idx ? class_idx + i : nullptr, label_id ? label_id + i : nullptr);
}

inline int wgs_per_image(int B, int HW) {
  const int tiles = ceil_div(HW, kTile), want = kTargetWgs / B > 0 ? kTargetWgs / B : 1;
  return tiles < want ? tiles : want;
}

template <int C, int KT>
void launch_vote(const float *y, const float *sem, int B, int T, int H, int W, int Hs, int Ws, int nwg, int vec_ok,
                 float *ws, hipStream_t st) {
  hipLaunchKernelGGL((vote_kernel<C, KT>), dim3(nwg, B), dim3(256), 0, st, y, sem, T, H * W, W, Hs, Ws, (double)Hs / (double)H,
                     (double)Ws / (double)W, ceil_div(H * W, kTile), vec_ok, ws);
}

}  // namespace icls
}  // namespace ra

using namespace ra;

static bool plane_ok(int H, int W) { return H > 0 && W > 0 && (long long)H * W <= (1ll << 30); }

extern "C" int ra_sem_foreground_f32(const float *sem, int B, int Hs, int Ws, int C, int H, int W, float thresh, float *fg,
                                     void *stream) {
  if (!sem || !fg || B <= 0) return fail(RA_E_INVALID, "ra_sem_foreground_f32: bad argument");
  if (!plane_ok(Hs, Ws) || !plane_ok(H, W) || C < 1 || C > icls::kMaxC || B > 65535)
    return fail(RA_E_SHAPE, "ra_sem_foreground_f32: sem %dx%dx%d -> %dx%d, B=%d (1 <= C <= %d, B <= 65535)", Hs, Ws, C, H, W,
                B, icls::kMaxC);
  const float lim = (float)(1.0 - (double)thresh);
  hipLaunchKernelGGL(icls::sem_foreground_kernel, dim3(ceil_div(H * W, 256), B), dim3(256), 0, as_stream(stream), sem, Hs, Ws,
                     C, H, W, (double)Hs / (double)H, (double)Ws / (double)W, thresh, lim, fg);
  return launch_status("ra_sem_foreground_f32");
}

extern "C" size_t ra_instance_class_vote_workspace_floats(int B, int T, int H, int W, int C) {
  if (B <= 0 || T <= 0 || C <= 0 || !plane_ok(H, W)) return 0;
  return (size_t)B * icls::wgs_per_image(B, H * W) * T * C;
}

extern "C" int ra_instance_class_vote_f32(const float *y, const float *sem, int B, int T, int H, int W, int Hs, int Ws,
                                          int C, const float *conf, float *ws, size_t ws_floats, float *vote,
                                          int *class_idx, int *label_id, void *stream) {
  if (!y || !sem || !ws || !vote || B <= 0) return fail(RA_E_INVALID, "ra_instance_class_vote_f32: bad argument");
  if (!conf && (class_idx || label_id))
    return fail(RA_E_INVALID, "ra_instance_class_vote_f32: class_idx / label_id need conf");
  if (T < 1 || T > icls::kMaxT || C < 2 || C > icls::kMaxC || !plane_ok(H, W) || !plane_ok(Hs, Ws) || B > 65535)
    return fail(RA_E_SHAPE, "ra_instance_class_vote_f32: T=%d C=%d y %dx%d sem %dx%d B=%d (1 <= T <= %d, 2 <= C <= %d, B <= 65535)",
                T, C, H, W, Hs, Ws, B, icls::kMaxT, icls::kMaxC);
  if (ws_floats < ra_instance_class_vote_workspace_floats(B, T, H, W, C))
    return fail(RA_E_WORKSPACE, "ra_instance_class_vote_f32: workspace");
  const int HW = H * W, nwg = icls::wgs_per_image(B, HW);
  const int vec_ok = HW % 4 == 0 && (reinterpret_cast<uintptr_t>(y) & 15) == 0;
  hipStream_t st = as_stream(stream);
  switch (C) {
#define RA_VOTE_CASE(c) \
  case c:               \
    if (T <= 20)        \
      icls::launch_vote<c, 5>(y, sem, B, T, H, W, Hs, Ws, nwg, vec_ok, ws, st); \
    else                \
      icls::launch_vote<c, icls::kTPerWave>(y, sem, B, T, H, W, Hs, Ws, nwg, vec_ok, ws, st); \
    break;
    RA_VOTE_CASE(2) RA_VOTE_CASE(3) RA_VOTE_CASE(4) RA_VOTE_CASE(5) RA_VOTE_CASE(6) RA_VOTE_CASE(7) RA_VOTE_CASE(8)
    RA_VOTE_CASE(9) RA_VOTE_CASE(10) RA_VOTE_CASE(11) RA_VOTE_CASE(12) RA_VOTE_CASE(13) RA_VOTE_CASE(14)
    RA_VOTE_CASE(15) RA_VOTE_CASE(16)
#undef RA_VOTE_CASE
  }
  if (int rc = launch_status("ra_instance_class_vote_f32")) return rc;
  hipLaunchKernelGGL(icls::vote_finish_kernel, dim3(T, B), dim3(256), 0, st, ws, nwg, T, C, 1.0 / (double)HW, conf, vote,
                     class_idx, label_id);
  return launch_status("ra_instance_class_vote_f32 (finish)");
}

extern "C" int ra_instance_class_pick_f32(const float *vote, const float *conf, int B, int T, int C, int *class_idx,
                                          int *label_id, void *stream) {
  if (!vote || !conf || (!class_idx && !label_id) || B <= 0)
    return fail(RA_E_INVALID, "ra_instance_class_pick_f32: bad argument");
  if (T < 1 || T > icls::kMaxT || C < 2 || C > icls::kMaxC)
    return fail(RA_E_SHAPE, "ra_instance_class_pick_f32: T=%d C=%d (1 <= T <= %d, 2 <= C <= %d)", T, C, icls::kMaxT,
                icls::kMaxC);
  hipLaunchKernelGGL(icls::pick_kernel, dim3(ceil_div(B * T, 256)), dim3(256), 0, as_stream(stream), vote, conf, B * T, C,
                     class_idx, label_id);
  return launch_status("ra_instance_class_pick_f32");
}
