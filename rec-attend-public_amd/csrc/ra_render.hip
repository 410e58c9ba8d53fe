// K23 — the render stage behind the evaluators: the colour images the reference's analyzers end in (analysis.py:95-193,
// 270-283), composed on the device while the masks are there.  Images are uint8 [B,H,W,3] in the memory order
// cv2.imwrite takes (B, G, R), the convention of utils/png.read_colour8.
//
//   instances    analysis.py:137-147 (RA_RENDER_ADD) and :166-187 (RA_RENDER_FIRST): every plane of y [B,T,H,W] cast to
//                uint8 and multiplied with its colour, summed in uint8 (ADD: both the product and the += wrap) or laid
//                under what is there (FIRST: a channel is written only while it is still 0, PER CHANNEL).  A lane owns four
//                consecutive pixels: one 16-byte load per plane, the loads of a group of kDepth planes issued before the
//                arithmetic of the group in front of it, and 12 output bytes as three dwords.  y is
//                read once, the image written once, nothing else: no atomics, no workspace.  The colour of a plane is the
//                same in every lane: the image's table waits in LDS, one packed word per plane.
//   orientation  fg_model_eval.py:128-132,154-164 with data_api/orientation.py:13-28: every channel of d [B,Hs,Ws,C] resized
//                to H x W (cv2.resize INTER_LINEAR, float32, the coordinate in double), the first maximum over the channels,
//                its wheel colour times the mask.  The arg-max is resample::argmax_channel_at, the device function behind
//                ra_sem_labels_u8; no full-size plane of d is written.  One thread per pixel, so that neighbouring lanes
//                share taps; the 768 bytes of a workgroup's 256 pixels change hands in LDS and leave as 192 dwords.
#include <cstdint>

#include "ra_common.h"
#include "ra_resample.h"

namespace ra {
namespace render {

typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr int kDepth = 4;   // planes whose loads are in flight together, twice that across a group boundary
constexpr int kMinC = 2, kMaxC = 16;

// the reference's .astype('uint8') of a finite 0 <= v <= 255
__device__ __forceinline__ unsigned u8_of(float v) { return (unsigned)(int)v & 255u; }

template <bool VEC>
__device__ __forceinline__ f32x4 load4(const float *q, unsigned p, unsigned HW) {
  f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
  if (VEC) {  // H * W % 4 == 0 and 16-byte aligned: p < HW implies p + 3 < HW
    v = __builtin_nontemporal_load(reinterpret_cast<const f32x4 *>(q + p));
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (p + j < HW) v[j] = q[p + j];
  }
  return v;
}

// Workgroup (x, b): lane l of it owns the pixels 4 * (256 x + l) .. + 3 of image b.  The image's colour table goes to LDS first,
// one packed word per plane: a colour read inside the t-loop then waits on the LDS counter only and leaves the planes' loads
// in flight (as global byte loads behind them, every colour made the wave wait for ALL its outstanding loads).
template <bool VEC, int MODE>
__global__ __launch_bounds__(256) void instances_kernel(const float *y, int T, unsigned HW, const unsigned char *colour,
                                                         unsigned char *img) {
  __shared__ unsigned sh_col[RA_RENDER_MAX_T];
  const int b = blockIdx.y;
  const unsigned p = 4u * (blockIdx.x * 256u + threadIdx.x);
  const bool live = p < HW;
  const float *yb = y + (size_t)b * T * HW;
  const f32x4 zero = f32x4{0.f, 0.f, 0.f, 0.f};
  f32x4 cur[kDepth], nxt[kDepth];
#pragma unroll
  for (int k = 0; k < kDepth; ++k) cur[k] = live && k < T ? load4<VEC>(yb + (size_t)k * HW, p, HW) : zero;
  const unsigned char *cb = colour + (size_t)b * T * 3;
  for (int t = threadIdx.x; t < T; t += 256) sh_col[t] = cb[3 * t] | cb[3 * t + 1] << 8 | cb[3 * t + 2] << 16;
  __syncthreads();
  if (!live) return;
  unsigned acc[4][3];
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j][0] = acc[j][1] = acc[j][2] = 0u;

  auto lay = [&](const f32x4 &v, int t) {  // plane t onto the lane's four pixels
    const unsigned col = sh_col[t], c0 = col & 255u, c1 = col >> 8 & 255u, c2 = col >> 16;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const unsigned u = u8_of(v[j]);
      if (MODE == RA_RENDER_ADD) {  // mod 256 once at the end: the sum of the wrapped products wraps to the same byte
        acc[j][0] += u * c0, acc[j][1] += u * c1, acc[j][2] += u * c2;
      } else {  // (total_img == 0) is an [H,W,3] array: decided per channel
        if (acc[j][0] == 0u) acc[j][0] = (u * c0) & 255u;
        if (acc[j][1] == 0u) acc[j][1] = (u * c1) & 255u;
        if (acc[j][2] == 0u) acc[j][2] = (u * c2) & 255u;
      }
    }
  };
  // Two groups per trip, cur and nxt changing roles without a copy (a register copy of nxt waits for its loads), and no branch
  // between a group's loads and the other group's arithmetic: the wait in front of that arithmetic then counts the kDepth younger
  // loads and leaves them in flight (behind a branch the compiler waits for every outstanding load).  The scheduling barriers
  // keep the loads where they are written; the scheduler otherwise sinks them below the arithmetic they are meant to cover.
  int t0 = 0;
  for (; t0 + 3 * kDepth <= T; t0 += 2 * kDepth) {
#pragma unroll
    for (int k = 0; k < kDepth; ++k) nxt[k] = load4<VEC>(yb + (size_t)(t0 + kDepth + k) * HW, p, HW);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int k = 0; k < kDepth; ++k) lay(cur[k], t0 + k);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int k = 0; k < kDepth; ++k) cur[k] = load4<VEC>(yb + (size_t)(t0 + 2 * kDepth + k) * HW, p, HW);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int k = 0; k < kDepth; ++k) lay(nxt[k], t0 + kDepth + k);
    __builtin_amdgcn_sched_barrier(0);
  }
  // what is left, fewer than 3 kDepth planes: cur holds the first group of them
#pragma unroll
  for (int k = 0; k < kDepth; ++k) nxt[k] = t0 + kDepth + k < T ? load4<VEC>(yb + (size_t)(t0 + kDepth + k) * HW, p, HW) : zero;
#pragma unroll
  for (int k = 0; k < kDepth; ++k)
    if (t0 + k < T) lay(cur[k], t0 + k);
#pragma unroll
  for (int k = 0; k < kDepth; ++k) cur[k] = t0 + 2 * kDepth + k < T ? load4<VEC>(yb + (size_t)(t0 + 2 * kDepth + k) * HW, p, HW) : zero;
#pragma unroll
  for (int k = 0; k < kDepth; ++k)
    if (t0 + kDepth + k < T) lay(nxt[k], t0 + kDepth + k);
#pragma unroll
  for (int k = 0; k < kDepth; ++k)
    if (t0 + 2 * kDepth + k < T) lay(cur[k], t0 + 2 * kDepth + k);

  unsigned char *o = img + ((size_t)b * HW + p) * 3;
  if (VEC) {  // img 4-byte aligned and H * W % 4 == 0: (b * HW + p) * 3 is a multiple of 12
    unsigned by[12];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int k = 0; k < 3; ++k) by[3 * j + k] = acc[j][k] & 255u;
    unsigned *o4 = reinterpret_cast<unsigned *>(o);
#pragma unroll
    for (int w = 0; w < 3; ++w) o4[w] = by[4 * w] | by[4 * w + 1] << 8 | by[4 * w + 2] << 16 | by[4 * w + 3] << 24;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (p + j < HW) {
#pragma unroll
        for (int k = 0; k < 3; ++k) o[3 * j + k] = (unsigned char)(acc[j][k] & 255u);
      }
  }
}

// One thread per output pixel, workgroup (x, b) the pixels 256 x .. 256 x + 255 of image b.
template <bool VEC>
__global__ __launch_bounds__(256) void orientation_kernel(const float *d, int Hs, int Ws, int C, double sy, double sx,
                                                           const float *mask, unsigned HW, int W, const unsigned char *wheel,
                                                           unsigned char *img) {
  __shared__ __attribute__((aligned(4))) unsigned char sh[256 * 3];
  const int b = blockIdx.y, tid = threadIdx.x;
  const unsigned base = blockIdx.x * 256u, e = base + tid;
  unsigned char px[3] = {0, 0, 0};
  if (e < HW) {
    const int r = (int)(e / (unsigned)W), c = (int)(e - (unsigned)r * (unsigned)W);
    const int cls = resample::argmax_channel_at(d + (size_t)b * Hs * Ws * C, Hs, Ws, C, sy, sx, r, c);
    const float m = mask[(size_t)b * HW + e];
#pragma unroll
    for (int k = 0; k < 3; ++k) px[k] = (unsigned char)u8_of((float)wheel[3 * cls + k] * m);  // (c2 * y).astype('uint8')
  }
  unsigned char *o = img + ((size_t)b * HW + base) * 3;
  if (VEC) {  // img 4-byte aligned and H * W % 4 == 0: the workgroup's bytes are whole dwords
#pragma unroll
    for (int k = 0; k < 3; ++k) sh[3 * tid + k] = px[k];
    __syncthreads();
    const unsigned n = HW - base < 256u ? HW - base : 256u;  // a multiple of 4
    if ((unsigned)tid < n / 4 * 3) reinterpret_cast<unsigned *>(o)[tid] = reinterpret_cast<const unsigned *>(sh)[tid];
  } else if (e < HW) {
#pragma unroll
    for (int k = 0; k < 3; ++k) o[3 * tid + k] = px[k];
  }
}

inline bool plane_ok(int H, int W) { return H > 0 && W > 0 && (long long)H * W <= (1ll << 30); }

template <int MODE>
void launch_instances(const float *y, int B, int T, unsigned HW, const unsigned char *colour, unsigned char *img, bool vec,
                      hipStream_t st) {
  const dim3 grid((HW + 1023u) / 1024u, B);
  if (vec)
    hipLaunchKernelGGL((instances_kernel<true, MODE>), grid, dim3(256), 0, st, y, T, HW, colour, img);
  else
    hipLaunchKernelGGL((instances_kernel<false, MODE>), grid, dim3(256), 0, st, y, T, HW, colour, img);
}

}  // namespace render
}  // namespace ra

using namespace ra;

extern "C" int ra_render_instances_u8(const float *y, int B, int T, int H, int W, const unsigned char *colour, int mode,
                                      unsigned char *img, void *stream) {
  if (!y || !colour || !img || B <= 0) return fail(RA_E_INVALID, "ra_render_instances_u8: bad argument");
  if (mode != RA_RENDER_ADD && mode != RA_RENDER_FIRST)
    return fail(RA_E_INVALID, "ra_render_instances_u8: mode %d (RA_RENDER_ADD or RA_RENDER_FIRST)", mode);
  if (T < 1 || T > RA_RENDER_MAX_T || !render::plane_ok(H, W) || B > 65535)
    return fail(RA_E_SHAPE, "ra_render_instances_u8: T=%d y %dx%d B=%d (1 <= T <= %d, planes up to 2^30 pixels, B <= 65535)", T, H,
                W, B, RA_RENDER_MAX_T);
  const unsigned HW = (unsigned)H * (unsigned)W;
  const bool vec = HW % 4 == 0 && (reinterpret_cast<uintptr_t>(y) & 15) == 0 && (reinterpret_cast<uintptr_t>(img) & 3) == 0;
  if (mode == RA_RENDER_ADD)
    render::launch_instances<RA_RENDER_ADD>(y, B, T, HW, colour, img, vec, as_stream(stream));
  else
    render::launch_instances<RA_RENDER_FIRST>(y, B, T, HW, colour, img, vec, as_stream(stream));
  return launch_status("ra_render_instances_u8");
}

extern "C" int ra_render_orientation_u8(const float *d, int B, int Hs, int Ws, int C, const float *mask, int H, int W,
                                        const unsigned char *wheel, unsigned char *img, void *stream) {
  if (!d || !mask || !wheel || !img || B <= 0) return fail(RA_E_INVALID, "ra_render_orientation_u8: bad argument");
  if (!render::plane_ok(Hs, Ws) || !render::plane_ok(H, W) || C < render::kMinC || C > render::kMaxC || B > 65535 ||
      (long long)Hs * Ws * C >= (1ll << 31))
    return fail(RA_E_SHAPE, "ra_render_orientation_u8: d %dx%dx%d -> %dx%d, B=%d (%d <= C <= %d, planes up to 2^30 pixels, B <= 65535)",
                Hs, Ws, C, H, W, B, render::kMinC, render::kMaxC);
  const unsigned HW = (unsigned)H * (unsigned)W;
  const double sy = (double)Hs / (double)H, sx = (double)Ws / (double)W;
  const dim3 grid((HW + 255u) / 256u, B);
  if (HW % 4 == 0 && (reinterpret_cast<uintptr_t>(img) & 3) == 0)
    hipLaunchKernelGGL(render::orientation_kernel<true>, grid, dim3(256), 0, as_stream(stream), d, Hs, Ws, C, sy, sx, mask, HW, W,
                       wheel, img);
  else
    hipLaunchKernelGGL(render::orientation_kernel<false>, grid, dim3(256), 0, as_stream(stream), d, Hs, Ws, C, sy, sx, mask, HW, W,
                       wheel, img);
  return launch_status("ra_render_orientation_u8");
}
