// K29 — pictures on the id path of the evaluator: the colour images of analysis.py:137-147 (RenderInstanceAnalyzer) and
// :166-187 (RenderGroundtruthInstanceAnalyzer), which full_model_eval.py:65-79,139-140 composes from [B,T,Hf,Wf] masks, painted
// from what the counting pass of ra_instance_eval.hip leaves behind instead: its winner map, one uint16 word n << 8 | t* per
// full-size pixel.  After apply_one_label a pixel belongs to at most one prediction t*, and it passes exactly the n smallest
// thresholds, so the sum over t of uint8(mask_t) * colour_t of the reference is ONE table row: colour[t*] where the threshold is
// passed, black elsewhere.  No mask plane exists on this route; a picture is a lookup, bound by the bytes it writes.
//
//   paint     paint_kernel<GEO>: a lane owns four consecutive pixels of one image — the map read once, 4 words as 8 bytes, and
//             per picture k (1 .. 16 of them, one per threshold) 12 bytes out as three dwords: colour[b,k,t*] where n > pos[k]
//             (pos: inse::Order's rank of threshold k among the call's thresholds), else 0.  A prediction remove_tiny took is a
//             zeroed colour row, set by the caller from the counted areas.
//   gt paint  gt_paint_kernel<GEO>: the ground truth's picture straight from the id image — the first slot whose inst_id equals
//             the pixel's id gives the colour, black where no slot lists it or the id is negative: RA_RENDER_FIRST on the
//             disjoint planes the ids define, without the planes.  16 bytes of ids in, 12 bytes out per lane.
// Both are templates over the geometry source of ra_ragged.h: workgroup (x, b) reads its image's table entry once, the grid's x
// extent follows the largest image and a workgroup beyond its own image's pixels does nothing; the elements between the images
// of a ragged batch are never written.  The colour tables of an image wait in LDS, one packed word per row, as in ra_render.hip.
// The wide forms need what instances_kernel's VEC needs, per image: the image's first element and its pixel count multiples of
// 4, the input aligned for its vector load, the output 4-byte aligned (and, picture by picture, its first byte 3 k P too: the
// pictures of a ragged batch whose element count is no multiple of 4 alternate).  An image that misses takes element loads and
// byte stores; its neighbours do not.
// Integer lookups only: no floating-point arithmetic in this file.
#include <cstdint>

#include "ra_common.h"
#include "ra_ragged.h"

namespace ra {
namespace paint {

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

constexpr int kMaxK = RA_INS_EVAL_MAX_K;  // 16 pictures per call
constexpr int kMaxT = RA_LABELS_MAX_T;    // 32
constexpr long long kMaxPixels = 1ll << 24;

struct Pos {
  int pos[kMaxK];
};

// 4 packed colours (byte 0 .. 2 of each word) -> the lane's 12 bytes at o; wide: three dwords, else the bytes of the first `live`
__device__ __forceinline__ void store4(unsigned char *o, const unsigned (&col)[4], bool wide, unsigned live) {
  if (wide) {
    unsigned *o4 = reinterpret_cast<unsigned *>(o);
    o4[0] = col[0] | col[1] << 24;
    o4[1] = col[1] >> 8 | col[2] << 16;
    o4[2] = col[2] >> 16 | col[3] << 8;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if ((unsigned)j < live) {
        o[3 * j] = (unsigned char)(col[j] & 255u);
        o[3 * j + 1] = (unsigned char)(col[j] >> 8 & 255u);
        o[3 * j + 2] = (unsigned char)(col[j] >> 16);
      }
  }
}

// colour [B,Kp,T,3]; out: picture k of image b from byte 3 * (k * P + im.off) on.  im.vec: the image takes the wide forms.
template <class GEO>
__global__ __launch_bounds__(256) void paint_kernel(const unsigned short *map, const GEO src, const Pos order, int Kp, int T,
                                                     const unsigned char *colour, unsigned char *out, size_t P) {
  __shared__ unsigned sh_col[kMaxK * kMaxT];
  __shared__ int sh_pos[kMaxK];
  const int b = blockIdx.y, tid = threadIdx.x;
  const geo::Image im = src.at(b);
  const unsigned HW = (unsigned)im.h * (unsigned)im.w;  // <= 2^24
  if (blockIdx.x * 1024u >= HW) return;                  // the whole workgroup: beyond its image
  const unsigned char *cb = colour + (size_t)b * Kp * T * 3;
  for (int i = tid; i < Kp * T; i += 256) sh_col[i] = cb[3 * i] | cb[3 * i + 1] << 8 | cb[3 * i + 2] << 16;
  if (tid < kMaxK) sh_pos[tid] = order.pos[tid];
  __syncthreads();
  const unsigned p = 4u * (blockIdx.x * 256u + tid);
  if (p >= HW) return;
  const bool wide = im.vec != 0;  // HW % 4 == 0: p + 3 < HW
  const unsigned live = HW - p < 4u ? HW - p : 4u;
  const unsigned short *mp = map + im.off + p;
  unsigned word[4] = {0u, 0u, 0u, 0u};
  if (wide) {
    const u32x2 q = *reinterpret_cast<const u32x2 *>(mp);
    word[0] = q[0] & 0xffffu, word[1] = q[0] >> 16, word[2] = q[1] & 0xffffu, word[3] = q[1] >> 16;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if ((unsigned)j < live) word[j] = mp[j];
  }
  int n[4], t[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    n[j] = (int)(word[j] >> 8);
    t[j] = (int)(word[j] & 255u);
    if (t[j] >= T) n[j] = 0, t[j] = 0;  // no word of the counting pass: black, and no read beyond the table
  }
  for (int k = 0; k < Kp; ++k) {
    const int pk = sh_pos[k];
    unsigned col[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) col[j] = n[j] > pk ? sh_col[k * T + t[j]] : 0u;
    // picture k starts at byte 3 k P: three dwords only where that is a multiple of 4 (decided per picture, not per lane)
    store4(out + 3 * ((size_t)k * P + (size_t)im.off + p), col, wide && ((size_t)k * P) % 4 == 0, live);
  }
}

// colour [B,T,3]; out [as gt_ids, 3]
template <class GEO>
__global__ __launch_bounds__(256) void gt_paint_kernel(const int *gt_ids, const int *inst_id, const GEO src, int T,
                                                        const unsigned char *colour, unsigned char *out) {
  __shared__ unsigned sh_col[kMaxT];
  __shared__ int sid[kMaxT];
  const int b = blockIdx.y, tid = threadIdx.x;
  const geo::Image im = src.at(b);
  const unsigned HW = (unsigned)im.h * (unsigned)im.w;
  if (blockIdx.x * 1024u >= HW) return;
  const unsigned char *cb = colour + (size_t)b * T * 3;
  if (tid < kMaxT) {
    sid[tid] = tid < T ? inst_id[(size_t)b * T + tid] : -1;
    sh_col[tid] = tid < T ? cb[3 * tid] | cb[3 * tid + 1] << 8 | cb[3 * tid + 2] << 16 : 0u;
  }
  __syncthreads();
  const unsigned p = 4u * (blockIdx.x * 256u + tid);
  if (p >= HW) return;
  const bool wide = im.vec != 0;
  const unsigned live = HW - p < 4u ? HW - p : 4u;
  const int *gp = gt_ids + im.off + p;
  int id[4] = {-1, -1, -1, -1};
  if (wide) {
    const i32x4 q = *reinterpret_cast<const i32x4 *>(gp);
#pragma unroll
    for (int j = 0; j < 4; ++j) id[j] = q[j];
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if ((unsigned)j < live) id[j] = gp[j];
  }
  unsigned col[4] = {0u, 0u, 0u, 0u};
  for (int s = T - 1; s >= 0; --s) {  // downwards: the first slot that lists the id remains
    const int want = sid[s];
    const unsigned c = sh_col[s];
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (want == id[j] && want >= 0) col[j] = c;
  }
  store4(out + 3 * ((size_t)im.off + p), col, wide, live);
}

inline unsigned grid_x(long long max_px) { return (unsigned)((max_px + 1023) / 1024); }

inline int check_pos(const char *who, const int *pos, int Kp, int T, Pos &order) {
  if (Kp < 1 || Kp > kMaxK) return fail(RA_E_SHAPE, "%s: Kp=%d pictures (1 .. %d)", who, Kp, kMaxK);
  if (T < 1 || T > kMaxT) return fail(RA_E_SHAPE, "%s: T=%d (1 .. %d)", who, T, kMaxT);
  for (int k = 0; k < kMaxK; ++k) {
    order.pos[k] = k < Kp ? pos[k] : kMaxK;
    if (k < Kp && (pos[k] < 0 || pos[k] >= kMaxK))
      return fail(RA_E_SHAPE, "%s: pos[%d] = %d (0 .. %d: how many thresholds lie below this one)", who, k, pos[k], kMaxK - 1);
  }
  return 0;
}

}  // namespace paint
}  // namespace ra

using namespace ra;

extern "C" int ra_instance_paint_u8(const unsigned short *map, int B, int Hf, int Wf, const int *pos, int Kp, int T,
                                    const unsigned char *colour, unsigned char *out, void *stream) {
  const char *who = "ra_instance_paint_u8";
  if (!map || !pos || !colour || !out || B <= 0 || Hf <= 0 || Wf <= 0) return fail(RA_E_INVALID, "%s: bad argument", who);
  paint::Pos order;
  if (int rc = paint::check_pos(who, pos, Kp, T, order)) return rc;
  if ((long long)Hf * Wf > paint::kMaxPixels || B > 65535)
    return fail(RA_E_SHAPE, "%s: %dx%d, B=%d (Hf * Wf <= 2^24, B <= 65535)", who, Hf, Wf, B);
  const long long HW = (long long)Hf * Wf;
  const int vec = HW % 4 == 0 && (reinterpret_cast<uintptr_t>(map) & 7) == 0 && (reinterpret_cast<uintptr_t>(out) & 3) == 0;
  hipLaunchKernelGGL(paint::paint_kernel<geo::Uniform>, dim3(paint::grid_x(HW), B), dim3(256), 0, as_stream(stream), map,
                     geo::Uniform{Hf, Wf, vec}, order, Kp, T, colour, out, (size_t)B * HW);
  return launch_status(who);
}

extern "C" int ra_instance_paint_ragged_u8(const unsigned short *map, size_t total, const ra_image_geo *geo, ra_image_geo *geo_dev,
                                           int B, const int *pos, int Kp, int T, const unsigned char *colour, unsigned char *out,
                                           void *stream) {
  const char *who = "ra_instance_paint_ragged_u8";
  if (!map || !geo || !geo_dev || !pos || !colour || !out || B <= 0) return fail(RA_E_INVALID, "%s: bad argument", who);
  paint::Pos order;
  if (int rc = paint::check_pos(who, pos, Kp, T, order)) return rc;
  if (B > 65535) return fail(RA_E_SHAPE, "%s: B=%d (B <= 65535)", who, B);
  if (int rc = geo::check(who, geo, B, total, paint::kMaxPixels, "h * w <= 2^24")) return rc;
  hipStream_t st = as_stream(stream);
  if (int rc = geo::upload(who, geo, geo_dev, B, st)) return rc;
  // geo::Ragged adds the image's share: w % 4 == 0 (so h * w % 4 == 0) and offset % 4 == 0
  const int vec = (reinterpret_cast<uintptr_t>(map) & 7) == 0 && (reinterpret_cast<uintptr_t>(out) & 3) == 0;
  hipLaunchKernelGGL(paint::paint_kernel<geo::Ragged>, dim3(paint::grid_x(geo::max_pixels(geo, B)), B), dim3(256), 0, st, map,
                     geo::Ragged{geo_dev, vec}, order, Kp, T, colour, out, total);
  return launch_status(who);
}

extern "C" int ra_gt_paint_u8(const int *gt_ids, const int *inst_id, int B, int T, int Hf, int Wf, const unsigned char *colour,
                              unsigned char *out, void *stream) {
  const char *who = "ra_gt_paint_u8";
  if (!gt_ids || !inst_id || !colour || !out || B <= 0 || Hf <= 0 || Wf <= 0) return fail(RA_E_INVALID, "%s: bad argument", who);
  if (T < 1 || T > paint::kMaxT) return fail(RA_E_SHAPE, "%s: T=%d (1 .. %d)", who, T, paint::kMaxT);
  if ((long long)Hf * Wf > paint::kMaxPixels || B > 65535)
    return fail(RA_E_SHAPE, "%s: %dx%d, B=%d (Hf * Wf <= 2^24, B <= 65535)", who, Hf, Wf, B);
  const long long HW = (long long)Hf * Wf;
  const int vec = HW % 4 == 0 && (reinterpret_cast<uintptr_t>(gt_ids) & 15) == 0 && (reinterpret_cast<uintptr_t>(out) & 3) == 0;
  hipLaunchKernelGGL(paint::gt_paint_kernel<geo::Uniform>, dim3(paint::grid_x(HW), B), dim3(256), 0, as_stream(stream), gt_ids,
                     inst_id, geo::Uniform{Hf, Wf, vec}, T, colour, out);
  return launch_status(who);
}

extern "C" int ra_gt_paint_ragged_u8(const int *gt_ids, size_t total, const ra_image_geo *geo, ra_image_geo *geo_dev,
                                     const int *inst_id, int B, int T, const unsigned char *colour, unsigned char *out,
                                     void *stream) {
  const char *who = "ra_gt_paint_ragged_u8";
  if (!gt_ids || !geo || !geo_dev || !inst_id || !colour || !out || B <= 0) return fail(RA_E_INVALID, "%s: bad argument", who);
  if (T < 1 || T > paint::kMaxT) return fail(RA_E_SHAPE, "%s: T=%d (1 .. %d)", who, T, paint::kMaxT);
  if (B > 65535) return fail(RA_E_SHAPE, "%s: B=%d (B <= 65535)", who, B);
  if (int rc = geo::check(who, geo, B, total, paint::kMaxPixels, "h * w <= 2^24")) return rc;
  hipStream_t st = as_stream(stream);
  if (int rc = geo::upload(who, geo, geo_dev, B, st)) return rc;
  const int vec = (reinterpret_cast<uintptr_t>(gt_ids) & 15) == 0 && (reinterpret_cast<uintptr_t>(out) & 3) == 0;
  hipLaunchKernelGGL(paint::gt_paint_kernel<geo::Ragged>, dim3(paint::grid_x(geo::max_pixels(geo, B)), B), dim3(256), 0, st, gt_ids,
                     inst_id, geo::Ragged{geo_dev, vec}, T, colour, out);
  return launch_status(who);
}
