// K24 — the Cityscapes output stage behind an EXTERNAL semantic segmentation given as a label image: the reference's
// --lrr_seg path (cityscapes_eval.py:162-164, 212-232) with any labelIds / trainIds / LRR image in place of its .mat files.
// There the label image becomes a one-hot [H,W,9] map, the foreground mask is "one of the eight thing classes", and the vote
// of an instance (analysis.py:235-237) is, per class, the share of the image's pixels that lie under its mask and carry that
// class: integer counting.  So the whole threshold loop (:183-189) collapses into
//
//   sweep_kernel    one read of y [B,T,H,W] for all K thresholds: per pixel the arg-max instance t* (first maximum,
//                   postprocess.py:45), its value v, the class c = lut[label]; a foreground pixel is binned ONCE, by
//                   (number of thresholds it passes, t*, c), into an LDS histogram, flushed once per workgroup with integer
//                   atomics.  Integers: exact at any size (a float32 count stops being exact at 2^24 pixels) and the same bits
//                   in any order.
//   finish_kernel   one thread per (b, t): suffix sums over the bins give the counts per threshold, taken back into the
//                   list's order; then sizes, remove_tiny with conf carried from threshold to threshold (:188-189,
//                   postprocess.py:130-133), the vote and the pick (analysis.py:232-261), walking the list in order.
//   planes_kernel   one threshold's binary planes, one read and one write: apply_one_label -> apply_threshold ->
//                   mask_foreground -> remove_tiny (postprocess.py:5-52, 109-145) fused.
//
// The thresholds reach the sweep sorted ascending (padded with +inf), so "the number of thresholds passed" n is a prefix and a
// pixel of bin n passes exactly the n smallest; the strict float32 comparison v > (float)threshold is postprocess.py:12 on a
// float32 array.  The 256-byte LUT and the thresholds are kernel arguments (by value): no device copy, nothing to keep alive.
//
// Histogram layout: hist[(n - 1) * T * 8 + t * 8 + (c - 1)], at most 16 x 32 x 8 int32 = 16 KB; pixels that pass no threshold
// or are background are not counted at all.  A lane merges its equal neighbours (4 consecutive pixels mostly share t*, c and
// n) before the LDS add; the lanes of a wave that then hit one address serialise in the LDS — at most 4 such adds per wave
// and tile of 1024 pixels, against T KB of loads per wave: a few per cent of the tile's memory time.
#include <cmath>
#include <cstdint>

#include "ra_common.h"
#include "ra_gt_ids.h"

namespace ra {
namespace lvote {

typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr int kMaxT = 32;     // the evaluator's limit (ra_eval.hip)
constexpr int kMaxK = 16;     // thresholds per sweep
constexpr int kClasses = gtid::kCsClasses;
constexpr int kTile = 1024;   // pixels per tile: 256 lanes x 4 consecutive pixels
constexpr int kTargetWgs = 2048;  // eight workgroups per CU: 4 x 16-byte loads in flight per lane hide HBM's latency
constexpr int kFinishThreads = 64;

struct Lut { unsigned w[64]; };               // 256 bytes: label value -> 0 (background / ignored) or 1 .. 8
struct Thresholds { float v[kMaxK]; };        // ascending, +inf beyond K
struct Order { unsigned char pos[kMaxK]; };   // pos[k]: where threshold k of the list stands in the sorted row

// The LUT into LDS, a byte per label value.  Indexed by constants only (a by-value argument indexed by the lane would be
// copied to scratch): thread i < 64 selects word i.
__device__ __forceinline__ void stage_lut(const Lut &lut, unsigned *sh) {
  const int tid = threadIdx.x;
  if (tid < 64) {
    unsigned v = 0;
#pragma unroll
    for (int i = 0; i < 64; ++i) v = tid == i ? lut.w[i] : v;
    sh[tid] = v;
  }
}

// This lane's 4 pixels at `base` of image b: the running maximum over t (first maximum wins) and the class of each.
__device__ __forceinline__ void argmax4(const float *yb, int T, int HW, int base, int vec_ok, f32x4 &best, int (&arg)[4]) {
  best = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < 4; ++j) arg[j] = 0;
  if (vec_ok) {  // H * W % 4 == 0 and 16-byte aligned: base < HW implies base + 3 < HW
    if (base >= HW) return;
    best = __builtin_nontemporal_load(reinterpret_cast<const f32x4 *>(yb + base));
#pragma unroll 4
    for (int t = 1; t < T; ++t) {
      const f32x4 v = __builtin_nontemporal_load(reinterpret_cast<const f32x4 *>(yb + (size_t)t * HW + base));
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (v[j] > best[j]) {  // strict: the first maximum, like numpy.argmax
          best[j] = v[j];
          arg[j] = t;
        }
    }
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (base + j < HW) best[j] = yb[base + j];
#pragma unroll 2
    for (int t = 1; t < T; ++t) {
      const float *q = yb + (size_t)t * HW + base;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (base + j < HW) {
          const float v = q[j];
          if (v > best[j]) {
            best[j] = v;
            arg[j] = t;
          }
        }
    }
  }
}

// the classes (0 = background, ignored or beyond the image) of the lane's 4 pixels
__device__ __forceinline__ void classes4(const unsigned char *lb, const unsigned char *lut_sh, int HW, int base, int lab_vec,
                                         int (&cls)[4]) {
  if (lab_vec) {  // H * W % 4 == 0 and 4-byte aligned
    unsigned w = 0;
    if (base < HW) w = *reinterpret_cast<const unsigned *>(lb + base);
#pragma unroll
    for (int j = 0; j < 4; ++j) cls[j] = base < HW ? lut_sh[(w >> (8 * j)) & 255u] : 0;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) cls[j] = base + j < HW ? lut_sh[lb[base + j]] : 0;
  }
}

// Workgroup (x, b) walks the tiles x, x + gridDim.x, ... of image b and leaves its histogram in bins [K,B,T,8]: bins[n - 1] =
// the pixels that pass exactly the n smallest thresholds.
__global__ __launch_bounds__(256) void sweep_kernel(const float *y, const unsigned char *labels, Lut lut, Thresholds th, int K,
                                                     int B, int T, int HW, int ntiles, int vec_ok, int lab_vec, int *bins) {
  extern __shared__ __attribute__((aligned(16))) int hist[];  // K * T * 8
  __shared__ unsigned lut_w[64];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int nhist = K * T * kClasses;
  stage_lut(lut, lut_w);
  for (int i = tid; i < nhist; i += 256) hist[i] = 0;
  __syncthreads();
  const unsigned char *lut_sh = reinterpret_cast<const unsigned char *>(lut_w);
  const float *yb = y + (size_t)b * T * HW;
  const unsigned char *lb = labels + (size_t)b * HW;

  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int base = tile * kTile + 4 * tid;
    f32x4 best;
    int arg[4], cls[4], key[4], cnt[4];
    classes4(lb, lut_sh, HW, base, lab_vec, cls);
    argmax4(yb, T, HW, base, vec_ok, best, arg);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      int n = 0;
#pragma unroll
      for (int k = 0; k < 8; ++k) n += best[j] > th.v[k] ? 1 : 0;
      if (K > 8) {
#pragma unroll
        for (int k = 8; k < kMaxK; ++k) n += best[j] > th.v[k] ? 1 : 0;
      }
      key[j] = cls[j] > 0 && n > 0 ? ((n - 1) * T + arg[j]) * kClasses + cls[j] - 1 : -1;
      cnt[j] = 1;
    }
#pragma unroll
    for (int j = 1; j < 4; ++j)
      if (key[j] >= 0 && key[j] == key[j - 1]) {  // equal neighbours: one add
        cnt[j] += cnt[j - 1];
        key[j - 1] = -1;
      }
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (key[j] >= 0) atomicAdd(&hist[key[j]], cnt[j]);
  }
  __syncthreads();
  for (int i = tid; i < nhist; i += 256) {
    const int v = hist[i];
    if (v) {
      const int n = i / (T * kClasses), r = i - n * T * kClasses;
      atomicAdd(&bins[((size_t)n * B + b) * T * kClasses + r], v);
    }
  }
}

// One thread per (b, t).  counts holds the sweep's bins on entry and the counts per threshold, in list order, on exit; the
// thread keeps its K x 8 numbers in LDS ([entry][thread]: no two threads on one bank) because the list's order indexes them.
__global__ __launch_bounds__(kFinishThreads) void finish_kernel(int *counts, Order order, int K, int B, int T, double inv_hw,
                                                                 const float *conf_in, int remove_tiny, int *sizes,
                                                                 unsigned char *keep, float *conf, float *vote, int *class_idx,
                                                                 int *label_id) {
  __shared__ int sh[kMaxK * kClasses][kFinishThreads];
  const int tid = threadIdx.x, inst = blockIdx.x * kFinishThreads + tid;
  if (inst >= B * T) return;
  const size_t BT = (size_t)B * T;
  for (int n = 0; n < K; ++n)
    for (int c = 0; c < kClasses; ++c) sh[n * kClasses + c][tid] = counts[((size_t)n * BT + inst) * kClasses + c];
  for (int n = K - 2; n >= 0; --n)  // bin n: exactly n + 1 passed -> at least n + 1 passed
    for (int c = 0; c < kClasses; ++c) sh[n * kClasses + c][tid] += sh[(n + 1) * kClasses + c][tid];
  float cf = conf_in[inst];
#pragma unroll
  for (int k = 0; k < kMaxK; ++k) {
    if (k < K) {
      const int p = order.pos[k];
      const size_t o = (size_t)k * BT + inst;
      int cnt[kClasses], size = 0;
#pragma unroll
      for (int c = 0; c < kClasses; ++c) {
        cnt[c] = sh[p * kClasses + c][tid];
        counts[o * kClasses + c] = cnt[c];
        size += cnt[c];
      }
      const bool kept = remove_tiny == 0 || size > remove_tiny;  // postprocess.py:115,131
      cf = kept ? cf : 0.f;                                      // :132, carried to the next threshold
      sizes[o] = size;
      keep[o] = kept ? 1 : 0;
      conf[o] = cf;
      float *v = vote + o * (kClasses + 1);
      v[0] = 0.f;  // no background pixel is left under a mask
      int idx = 0;
#pragma unroll
      for (int c = 0; c < kClasses; ++c) {
        v[1 + c] = kept ? (float)((double)cnt[c] * inv_hw) : 0.f;
        if (cnt[c] > cnt[idx]) idx = c;  // strict: the first maximum
      }
      const bool written = cf > 0.5f;  // analysis.py:232; the gate of :251 (vote[0] <= 0.7) is always open
      class_idx[o] = written ? idx : -1;
      label_id[o] = written ? gtid::cs_label_id(idx) : -1;
    }
  }
}

// One lane per 4 pixels: read the T planes, write the T planes.
__global__ __launch_bounds__(256) void planes_kernel(const float *y, const unsigned char *labels, Lut lut, float thresh,
                                                      const unsigned char *keep, int T, int HW, int vec_ok, int lab_vec,
                                                      float *y_bin) {
  __shared__ unsigned lut_w[64];
  const int b = blockIdx.y, tid = threadIdx.x;
  stage_lut(lut, lut_w);
  __syncthreads();
  const unsigned char *lut_sh = reinterpret_cast<const unsigned char *>(lut_w);
  const int base = blockIdx.x * kTile + 4 * tid;
  if (base >= HW) return;
  f32x4 best;
  int arg[4], cls[4];
  classes4(labels + (size_t)b * HW, lut_sh, HW, base, lab_vec, cls);
  argmax4(y + (size_t)b * T * HW, T, HW, base, vec_ok, best, arg);
  bool on[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) on[j] = cls[j] > 0 && best[j] > thresh;
  float *ob = y_bin + (size_t)b * T * HW + base;
  for (int t = 0; t < T; ++t) {
    const bool kept = keep ? keep[(size_t)b * T + t] != 0 : true;
    f32x4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = kept && on[j] && arg[j] == t ? 1.f : 0.f;
    float *q = ob + (size_t)t * HW;
    if (vec_ok) {
      __builtin_nontemporal_store(o, reinterpret_cast<f32x4 *>(q));
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (base + j < HW) q[j] = o[j];
    }
  }
}

inline int wgs_per_image(int B, int HW) {
  const int tiles = ceil_div(HW, kTile), want = kTargetWgs / B > 0 ? kTargetWgs / B : 1;
  return tiles < want ? tiles : want;
}

// the shared refusals; 0 when the shape may be launched
inline int check_shape(const char *who, const unsigned char *lut, int B, int T, int H, int W) {
  if (T < 1 || T > kMaxT || B > 65535 || H <= 0 || W <= 0 || (long long)H * W > (1ll << 30))
    return fail(RA_E_SHAPE, "%s: T=%d y %dx%d B=%d (1 <= T <= %d, B <= 65535, H * W <= 2^30)", who, T, H, W, B, kMaxT);
  for (int i = 0; i < 256; ++i)
    if (lut[i] > kClasses) return fail(RA_E_SHAPE, "%s: lut[%d] = %d (0 .. %d)", who, i, (int)lut[i], kClasses);
  return 0;
}

inline Lut pack_lut(const unsigned char *lut) {
  Lut l;
  for (int i = 0; i < 64; ++i)
    l.w[i] = (unsigned)lut[4 * i] | (unsigned)lut[4 * i + 1] << 8 | (unsigned)lut[4 * i + 2] << 16 | (unsigned)lut[4 * i + 3] << 24;
  return l;
}

}  // namespace lvote
}  // namespace ra

using namespace ra;

extern "C" int ra_label_vote_sweep_f32(const float *y, const unsigned char *labels, const unsigned char *lut, int B, int T,
                                       int H, int W, const double *thresholds, int K, const float *conf_in, int remove_tiny,
                                       int *counts, int *sizes, unsigned char *keep, float *conf, float *vote,
                                       int *class_idx, int *label_id, void *stream) {
  const char *who = "ra_label_vote_sweep_f32";
  if (!y || !labels || !lut || !thresholds || !conf_in || !counts || !sizes || !keep || !conf || !vote || !class_idx ||
      !label_id || B <= 0 || remove_tiny < 0)
    return fail(RA_E_INVALID, "%s: bad argument", who);
  if (K < 1 || K > lvote::kMaxK) return fail(RA_E_SHAPE, "%s: K=%d thresholds (1 <= K <= %d)", who, K, lvote::kMaxK);
  if (int rc = lvote::check_shape(who, lut, B, T, H, W)) return rc;
  // sorted ascending as float32 (a stable insertion sort: equal thresholds keep the list's order; either gives the same counts)
  lvote::Thresholds th;
  lvote::Order order;
  int by[lvote::kMaxK];
  for (int k = 0; k < K; ++k) {
    if (std::isnan(thresholds[k])) return fail(RA_E_INVALID, "%s: thresholds[%d] is not a number", who, k);
    const float v = (float)thresholds[k];
    int i = k;
    for (; i > 0 && th.v[i - 1] > v; --i) {
      th.v[i] = th.v[i - 1];
      by[i] = by[i - 1];
    }
    th.v[i] = v;
    by[i] = k;
  }
  for (int i = 0; i < lvote::kMaxK; ++i) {
    if (i < K) order.pos[by[i]] = (unsigned char)i;
    else th.v[i] = __builtin_inff(), order.pos[i] = 0;
  }
  const int HW = H * W;
  const int vec_ok = HW % 4 == 0 && (reinterpret_cast<uintptr_t>(y) & 15) == 0;
  const int lab_vec = HW % 4 == 0 && (reinterpret_cast<uintptr_t>(labels) & 3) == 0;
  hipStream_t st = as_stream(stream);
  const size_t n = (size_t)K * B * T * lvote::kClasses;
  if (hipError_t e = hipMemsetAsync(counts, 0, n * sizeof(int), st)) {
    set_error("%s: zeroing counts: %s", who, hipGetErrorString(e));
    return (int)e;
  }
  hipLaunchKernelGGL(lvote::sweep_kernel, dim3(lvote::wgs_per_image(B, HW), B), dim3(256),
                     (size_t)K * T * lvote::kClasses * sizeof(int), st, y, labels, lvote::pack_lut(lut), th, K, B, T, HW,
                     ceil_div(HW, lvote::kTile), vec_ok, lab_vec, counts);
  if (int rc = launch_status(who)) return rc;
  hipLaunchKernelGGL(lvote::finish_kernel, dim3(ceil_div(B * T, lvote::kFinishThreads)), dim3(lvote::kFinishThreads), 0, st,
                     counts, order, K, B, T, 1.0 / (double)HW, conf_in, remove_tiny, sizes, keep, conf, vote, class_idx,
                     label_id);
  return launch_status("ra_label_vote_sweep_f32 (finish)");
}

extern "C" int ra_label_planes_f32(const float *y, const unsigned char *labels, const unsigned char *lut, int B, int T, int H,
                                   int W, double thresh, const unsigned char *keep, float *y_bin, void *stream) {
  const char *who = "ra_label_planes_f32";
  if (!y || !labels || !lut || !y_bin || B <= 0 || std::isnan(thresh)) return fail(RA_E_INVALID, "%s: bad argument", who);
  if (int rc = lvote::check_shape(who, lut, B, T, H, W)) return rc;
  const int HW = H * W;
  const int vec_ok = HW % 4 == 0 && ((reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(y_bin)) & 15) == 0;
  const int lab_vec = HW % 4 == 0 && (reinterpret_cast<uintptr_t>(labels) & 3) == 0;
  hipLaunchKernelGGL(lvote::planes_kernel, dim3(ceil_div(HW, lvote::kTile), B), dim3(256), 0, as_stream(stream), y, labels,
                     lvote::pack_lut(lut), (float)thresh, keep, T, HW, vec_ok, lab_vec, y_bin);
  return launch_status(who);
}
