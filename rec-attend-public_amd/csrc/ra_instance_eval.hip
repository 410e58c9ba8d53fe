// K25 — the decode loop's evaluator at the labels' own size, from instance-id images, as ONE counting pass: the chain of
// full_model_eval.py:97-139 behind apply_confidence — upsample (postprocess.py:75-106) [-> morph (:55-72)] -> apply_one_label
// (:32-52) -> per threshold apply_threshold (:5-12) [-> mask_foreground (:139-147)] — ends in binary masks of which the
// analyzers (analysis.py:314-787) read three integer quantities only: the pairwise intersections, the predictions' areas and
// the ground truth's areas.  After one-label the predictions of an image are disjoint, and the instances of an id image are
// disjoint by construction, so every full-size pixel belongs to at most ONE (prediction t*, ground-truth slot j) pair per
// threshold: the chain reduces to a histogram, and no [., Hf, Wf] float plane is written anywhere.
//
//   count   count_kernel<MORPH>.  A workgroup owns tiles of kTH x kTW = 16 x 128 full-size pixels, the tile of
//           ra_fg_eval.hip's sweep_kernel, with the loop over the T instances INSIDE the tile.  Per instance t:
//             1. the resize (ra_resample.h) of the tile plus its halo into LDS: 2 pixels for the bilateral window, 2 more
//                with MORPH (the 5 x 5 dilation reads filtered values up to 2 pixels outside the tile, each of which reads
//                resized values 2 further out: 4 in all).  A halo coordinate goes through reflect101 in full-size
//                coordinates first, so LDS holds what the plane kernel bilateral5_kernel would fetch;
//             2. the bilateral filter, 4 consecutive pixels at a time from a 5 x 8 window read as ten ds_read_b128 (row
//                pitches are multiples of 4 floats).  Without MORPH a thread filters its own 2 x 4 pixels.  With MORPH the
//                threads first filter the 20 x 132 pixels the dilation reads into a second LDS tile — a pixel outside the
//                image becomes -inf there, which is how ra_dilate_f32 ignores it — and then take the maximum over the
//                5 x 5 window of their own pixels;
//             3. the fold into a running (best value, best index) pair per pixel in registers, with a strict `>`: the
//                lower index wins an exact tie, as postprocess_kernel's and numpy.argmax's first maximum.
//           Then one increment per pixel: the thresholds are sorted on the host, so bucket n = #{sorted thresholds below
//           the pixel's maximum m} (0 where fg masks the pixel) says everything — the pixel passes exactly the n smallest.
//           Its ground-truth slot j is the first slot whose inst_id equals its id (at most T compares against LDS, next to
//           13 T exponentials; no table indexed by id), T when no slot lists the id.  hist[n - 1][t*][j] in LDS takes the
//           pixel when n > 0, area[j] takes it when j < T.  Equal neighbours among a lane's 4 pixels share one LDS atomic.
//           LDS: 13 KB (24 KB with MORPH) of tiles, static, and (K T (T + 1) + T) * 4 bytes of histogram, dynamic and sized
//           by the call's own K and T: 3.4 KB at K = 1, T = 20, 17 KB at K = 10, T = 20 (three workgroups per CU with
//           MORPH), 68 KB at K = 16, T = 32 (one workgroup per CU: that corner pays in occupancy, not in correctness).
//           The workgroup's non-zero bins leave it as 32-bit integer atomics; the grid is capped (kWgs workgroups in all).
//   finish  finish_kernel: one thread per (image, t, j) turns "exactly n passed" into "at least n passed" by a suffix sum
//           over its K bins and writes them back in the order the thresholds were given, in place (a thread reads all of
//           its K numbers before it writes any, and no other thread touches them).
// Integer atomics only: the counts are the same bits on every run.  Hf * Wf <= 2^24 keeps every count exact in the float32
// that ra_eval_metrics_f32 takes.
// Mixed full sizes in one batch (ra_instance_eval_counts_ragged_f32): count_kernel is a template over the geometry source of
// ra_ragged.h — gt_ids and fg flat, image b at its table entry, read once per workgroup — and the same body runs either form.
// The winner map (ra_instance_eval_counts_map_f32 / _ragged_f32): count_kernel<.., MAP = true> also writes what it holds in
// registers when it increments — (t*, n) per pixel, as ONE uint16 word n << 8 | t* (0 where n == 0) at the pixel's element of
// gt_ids.  Every thresholded mask of every threshold is in it: threshold k as given is passed iff n > Order::pos[k].  A lane's 4
// pixels of a row leave as one 8-byte store where W % 4 == 0, the image starts at a multiple of 4 elements and map is 8-byte
// aligned (decided per image, as the loads are), as element stores otherwise.  No atomics, no LDS; the instantiations without
// the map are the ones the file had before.
#include <cstdint>

#include "ra_common.h"
#include "ra_ragged.h"
#include "ra_resample.h"

namespace ra {
namespace inse {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

constexpr int kMaxK = RA_INS_EVAL_MAX_K;  // 16
constexpr int kMaxT = RA_LABELS_MAX_T;    // 32
constexpr int kTH = 16, kTW = 128;        // the tile: 256 threads x 2 rows x 4 pixels
constexpr int kWgs = 1024;                // workgroups in all: four per CU
constexpr long long kMaxPixels = 1ll << 24;

struct Thresholds {
  float t[kMaxK];  // ascending, padded with +inf (which no value exceeds)
};
struct Order {
  int pos[kMaxK];  // pos[k]: how many of the thresholds lie strictly below the k-th one given
};

template <bool MORPH>
struct Geo {
  static constexpr int kHalo = MORPH ? 4 : 2;
  static constexpr int kRH = kTH + 2 * kHalo, kRW = kTW + 2 * kHalo;  // the resized tile; kRW % 4 == 0
  static constexpr int kFH = kTH + 4, kFW = kTW + 4;                  // the filtered tile the dilation reads (MORPH)
};

__host__ __device__ inline int tiles_x(int W) { return ceil_div(W, kTW); }
__host__ __device__ inline int tiles(int H, int W) { return ceil_div(H, kTH) * tiles_x(W); }
inline int grid_x(int B, int H, int W) {
  const int n = tiles(H, W), want = kWgs / B > 0 ? kWgs / B : 1;
  return n < want ? n : want;
}
inline size_t hist_ints(int K, int T) { return (size_t)K * T * (T + 1) + T; }

// The filtered values of the 4 pixels whose 5 x 5 windows are the rows 0 .. 4, columns 0 .. 7 at q0 (16-byte aligned, `pitch`
// floats per row, pitch % 4 == 0): pixel j is centred on row 2, column j + 2.
__device__ __forceinline__ void filter4(const float *q0, int pitch, float gs, float gc, float (&out)[4]) {
  f32x4 win[5][2];
#pragma unroll
  for (int dy = 0; dy < 5; ++dy) {
    const f32x4 *q = reinterpret_cast<const f32x4 *>(q0 + dy * pitch);
    win[dy][0] = q[0];
    win[dy][1] = q[1];
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const auto at = [&](int dy, int dx) {
      const int x = j + dx + 2;  // 0 .. 7, a constant after unrolling
      return win[dy + 2][x >> 2][x & 3];
    };
    out[j] = resample::bilateral5_at(at, at(0, 0), gs, gc);
  }
}

// The maxima over the 5 x 5 windows of the same 4 pixels (rows 0 .. 4, columns j .. j + 4 at q0).
__device__ __forceinline__ void dilate4(const float *q0, int pitch, float (&out)[4]) {
  f32x4 win[5][2];
#pragma unroll
  for (int dy = 0; dy < 5; ++dy) {
    const f32x4 *q = reinterpret_cast<const f32x4 *>(q0 + dy * pitch);
    win[dy][0] = q[0];
    win[dy][1] = q[1];
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float m = -__builtin_inff();
#pragma unroll
    for (int dy = 0; dy < 5; ++dy)
#pragma unroll
      for (int dx = 0; dx < 5; ++dx) {
        const int x = j + dx;
        m = fmaxf(m, win[dy][x >> 2][x & 3]);
      }
    out[j] = m;
  }
}

// adds cnt[j] to base[key[j]] for every key[j] >= 0; equal neighbours share one atomic
__device__ __forceinline__ void add4(int *base, int (&key)[4]) {
  int cnt[4] = {1, 1, 1, 1};
#pragma unroll
  for (int j = 1; j < 4; ++j)
    if (key[j] >= 0 && key[j] == key[j - 1]) {
      cnt[j] += cnt[j - 1];
      key[j - 1] = -1;
    }
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (key[j] >= 0) atomicAdd(&base[key[j]], cnt[j]);
}

// vec: W % 4 == 0 and gt_ids 16-byte, fg 4-byte aligned — a lane's 4 ids are one 16-byte load, its 4 fg bytes one 32-bit load
// GEO: geo::Uniform (gt_ids and fg are [B,H,W]) or geo::Ragged (both flat, image b at its table entry: its own H, W in the
// resize, in reflect101, in the in-image test and in the tile walk; a workgroup beyond its image's tiles adds nothing).
// MAP: map [as gt_ids] takes n << 8 | t* of every pixel of the image (0 where n == 0); mvec: its 4 words per lane are one store.
template <bool MORPH, class GEO, bool MAP>
__global__ __launch_bounds__(256) void count_kernel(const float *yc, const int *gt_ids, const int *inst_id,
                                                     const unsigned char *fg, int T, int Hs, int Ws, const GEO src,
                                                     const Thresholds thr, int K, int *inter, int *area_b, unsigned short *map) {
  using G = Geo<MORPH>;
  __shared__ __attribute__((aligned(16))) float rs[G::kRH * G::kRW];
  __shared__ __attribute__((aligned(16))) float fl[MORPH ? G::kFH * G::kFW : 4];
  __shared__ int sid[kMaxT];
  __shared__ float sthr[kMaxK];
  extern __shared__ __attribute__((aligned(16))) int hist[];  // [K][T][T + 1] | area [T]
  const int b = blockIdx.y, tid = threadIdx.x;
  const int tx = tid & 31, ty = tid >> 5;  // 4 pixels at column 4 tx of the rows ty and ty + 8
  const int T1 = T + 1, nbins = K * T * T1, nhist = nbins + T;
  for (int i = tid; i < nhist; i += 256) hist[i] = 0;
  if (tid < kMaxT) sid[tid] = tid < T ? inst_id[(size_t)b * T + tid] : -1;
  if (tid < kMaxK) sthr[tid] = thr.t[tid];
  const float gs = resample::bilateral_gain(10.f), gc = resample::bilateral_gain(10.f);  // postprocess.py:105
  const geo::Image im = src.at(b);
  const int H = im.h, W = im.w, vec = im.vec;
  const int *gp = gt_ids + im.off;
  const unsigned char *fp = fg ? fg + im.off : nullptr;
  unsigned short *mp = MAP ? map + im.off : nullptr;
  const bool mvec = MAP && W % 4 == 0 && im.off % 4 == 0 && (reinterpret_cast<uintptr_t>(map) & 7) == 0;
  const int ntx = tiles_x(W), ntiles = tiles(H, W);

  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int r0 = (tile / ntx) * kTH, c0 = (tile % ntx) * kTW;
    float best[2][4];
    int arg[2][4];
#pragma unroll
    for (int i = 0; i < 8; ++i) best[i >> 2][i & 3] = -__builtin_inff(), arg[i >> 2][i & 3] = 0;
    for (int t = 0; t < T; ++t) {
      const float *sp = yc + ((size_t)b * T + t) * Hs * Ws;
      __syncthreads();  // the readers of the previous instance's tiles are done (and hist / sid are set)
      for (int e = tid; e < G::kRH * G::kRW; e += 256) {
        const int ly = e / G::kRW, lx = e - ly * G::kRW;
        const int r = resample::reflect101(r0 + ly - G::kHalo, H), c = resample::reflect101(c0 + lx - G::kHalo, W);
        rs[e] = resample::resize_linear_at(sp, Hs, Ws, H, W, r, c);
      }
      __syncthreads();
      if (MORPH) {
        constexpr int kGroups = G::kFW / 4;  // 33 groups of 4 pixels per filtered row
        for (int g = tid; g < G::kFH * kGroups; g += 256) {
          const int fy = g / kGroups, gx = g - fy * kGroups;
          float o[4];
          filter4(rs + fy * G::kRW + 4 * gx, G::kRW, gs, gc, o);
          const int r = r0 + fy - 2, c = c0 + 4 * gx - 2;
          const bool row_in = r >= 0 && r < H;
          f32x4 v;
#pragma unroll
          for (int j = 0; j < 4; ++j) v[j] = row_in && c + j >= 0 && c + j < W ? o[j] : -__builtin_inff();
          *reinterpret_cast<f32x4 *>(fl + fy * G::kFW + 4 * gx) = v;
        }
        __syncthreads();
      }
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        const int row = ty + 8 * half;
        float v[4];
        if (MORPH)
          dilate4(fl + row * G::kFW + 4 * tx, G::kFW, v);
        else
          filter4(rs + row * G::kRW + 4 * tx, G::kRW, gs, gc, v);
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (v[j] > best[half][j]) {  // strict: the first maximum wins
            best[half][j] = v[j];
            arg[half][j] = t;
          }
      }
    }
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      const int r = r0 + ty + 8 * half, c = c0 + 4 * tx;
      const bool row_in = r < H;
      int id[4] = {-1, -1, -1, -1};
      unsigned f[4] = {1u, 1u, 1u, 1u};
      if (vec) {
        if (row_in && c < W) {  // W % 4 == 0: c + 3 < W
          const i32x4 q = *reinterpret_cast<const i32x4 *>(gp + (size_t)r * W + c);
          unsigned w = 0x01010101u;
          if (fp) w = *reinterpret_cast<const unsigned *>(fp + (size_t)r * W + c);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            id[j] = q[j];
            f[j] = (w >> (8 * j)) & 255u;
          }
        }
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (row_in && c + j < W) {
            id[j] = gp[(size_t)r * W + c + j];
            if (fp) f[j] = fp[(size_t)r * W + c + j];
          }
      }
      int slot[4] = {T, T, T, T};
      for (int s = T - 1; s >= 0; --s) {  // downwards: the first slot that lists the id remains
        const int want = sid[s];
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (want == id[j] && want >= 0) slot[j] = s;
      }
      int key_h[4], key_a[4];
      unsigned word[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool in = row_in && c + j < W;
        int n = 0;
#pragma unroll
        for (int k = 0; k < kMaxK; ++k) n += best[half][j] > sthr[k] ? 1 : 0;
        if (f[j] == 0u) n = 0;
        word[j] = n > 0 ? (unsigned)(n << 8 | arg[half][j]) : 0u;
        key_h[j] = in && n > 0 ? ((n - 1) * T + arg[half][j]) * T1 + slot[j] : -1;
        key_a[j] = in && slot[j] < T ? slot[j] : -1;
      }
      add4(hist, key_h);
      add4(hist + nbins, key_a);
      if (MAP) {
        if (mvec) {
          if (row_in && c < W)  // W % 4 == 0: c + 3 < W, and (off + r W + c) * 2 bytes is a multiple of 8
            *reinterpret_cast<u32x2 *>(mp + (size_t)r * W + c) = u32x2{word[0] | word[1] << 16, word[2] | word[3] << 16};
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (row_in && c + j < W) mp[(size_t)r * W + c + j] = (unsigned short)word[j];
        }
      }
    }
  }
  __syncthreads();
  int *ib = inter + (size_t)b * nbins;
  for (int i = tid; i < nhist; i += 256) {
    const int v = hist[i];
    if (v) atomicAdd(i < nbins ? ib + i : area_b + (size_t)b * T + (i - nbins), v);
  }
}

// inter [B,K,T,T + 1]: on entry bin n holds the pixels that pass exactly the n + 1 smallest thresholds, on exit slot k holds
// those that pass the k-th threshold given.
__global__ __launch_bounds__(256) void finish_kernel(int *inter, const Order order, int K, int TT1, int total) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int b = i / TT1, r = i - b * TT1;
  int *p = inter + (size_t)b * K * TT1 + r;
  int v[kMaxK];
#pragma unroll
  for (int n = 0; n < kMaxK; ++n) v[n] = n < K ? p[(size_t)n * TT1] : 0;
#pragma unroll
  for (int k = 0; k < kMaxK; ++k)
    if (k < K) {
      int s = 0;
#pragma unroll
      for (int n = 0; n < kMaxK; ++n) s += n >= order.pos[k] ? v[n] : 0;
      p[(size_t)k * TT1] = s;
    }
}


template <bool MORPH, class GEO, bool MAP>
void launch_count(dim3 grid, size_t lds, hipStream_t st, const float *yc, const int *gt_ids, const int *inst_id,
                  const unsigned char *fg, int T, int Hs, int Ws, const GEO &src, const Thresholds &thr, int K, int *inter,
                  int *area_b, unsigned short *map) {
  static const MaxDynamicLds raise{count_kernel<MORPH, GEO, MAP>, hist_ints(kMaxK, kMaxT) * sizeof(int)};
  hipLaunchKernelGGL((count_kernel<MORPH, GEO, MAP>), grid, dim3(256), lds, st, yc, gt_ids, inst_id, fg, T, Hs, Ws, src, thr, K,
                     inter, area_b, map);
}

// The checks both entry points share, and the thresholds sorted for the kernel.
inline int prepare(const char *who, int B, int T, int Hs, int Ws, const float *thresholds, int K, Thresholds &thr, Order &order) {
  if (K < 1 || K > kMaxK) return fail(RA_E_SHAPE, "%s: K=%d thresholds (1 .. %d)", who, K, kMaxK);
  if (T < 1 || T > kMaxT) return fail(RA_E_SHAPE, "%s: T=%d (1 .. %d)", who, T, kMaxT);
  float sorted[kMaxK];
  for (int k = 0; k < K; ++k) {
    if (!(thresholds[k] >= 0.f))
      return fail(RA_E_SHAPE, "%s: threshold %d is %g (>= 0: below zero the planes that lost the arg-max pass apply_threshold)",
                  who, k, (double)thresholds[k]);
    int i = k;  // insertion sort, ascending
    for (; i > 0 && sorted[i - 1] > thresholds[k]; --i) sorted[i] = sorted[i - 1];
    sorted[i] = thresholds[k];
  }
  for (int k = 0; k < kMaxK; ++k) {
    thr.t[k] = k < K ? sorted[k] : __builtin_inff();
    order.pos[k] = 0;
    if (k < K)
      for (int i = 0; i < K; ++i) order.pos[k] += thresholds[i] < thresholds[k] ? 1 : 0;
  }
  return 0;
}

// clear -> count -> finish on one stream; grid_x workgroups per image.  map: NULL, or the winner map the count pass also writes.
template <class GEO>
int launch_all(const char *who, const float *yc, const int *gt_ids, const int *inst_id, const unsigned char *fg, int B, int T,
               int Hs, int Ws, const GEO &src, int gx, int morph, const Thresholds &thr, const Order &order, int K, int *inter,
               int *area_b, unsigned short *map, hipStream_t st) {
  char what[96];
  const auto status = [&](const char *stage) {
    snprintf(what, sizeof(what), "%s%s", who, stage);
    return launch_status(what);
  };
  const int TT1 = T * (T + 1);
  if (hipMemsetAsync(inter, 0, (size_t)B * K * TT1 * sizeof(int), st) != hipSuccess ||
      hipMemsetAsync(area_b, 0, (size_t)B * T * sizeof(int), st) != hipSuccess)
    return status(" (clear)");
  const dim3 grid(gx, B);
  const size_t lds = hist_ints(K, T) * sizeof(int);
  if (morph && map)
    launch_count<true, GEO, true>(grid, lds, st, yc, gt_ids, inst_id, fg, T, Hs, Ws, src, thr, K, inter, area_b, map);
  else if (morph)
    launch_count<true, GEO, false>(grid, lds, st, yc, gt_ids, inst_id, fg, T, Hs, Ws, src, thr, K, inter, area_b, nullptr);
  else if (map)
    launch_count<false, GEO, true>(grid, lds, st, yc, gt_ids, inst_id, fg, T, Hs, Ws, src, thr, K, inter, area_b, map);
  else
    launch_count<false, GEO, false>(grid, lds, st, yc, gt_ids, inst_id, fg, T, Hs, Ws, src, thr, K, inter, area_b, nullptr);
  if (int rc = status("")) return rc;
  hipLaunchKernelGGL(finish_kernel, dim3(ceil_div(B * TT1, 256)), dim3(256), 0, st, inter, order, K, TT1, B * TT1);
  return status(" (finish)");
}

}  // namespace inse
}  // namespace ra

using namespace ra;

namespace {

int counts_uniform(const char *who, const float *yc, const int *gt_ids, const int *inst_id, const unsigned char *fg, int B, int T,
                   int Hs, int Ws, int Hf, int Wf, int morph, const float *thresholds, int K, int *inter, int *area_b,
                   unsigned short *map, void *stream) {
  if (!yc || !gt_ids || !inst_id || !thresholds || !inter || !area_b || B <= 0 || Hs <= 0 || Ws <= 0 || Hf <= 0 || Wf <= 0)
    return fail(RA_E_INVALID, "%s: bad argument", who);
  if (K < 1 || K > inse::kMaxK) return fail(RA_E_SHAPE, "%s: K=%d thresholds (1 .. %d)", who, K, inse::kMaxK);
  if (T < 1 || T > inse::kMaxT) return fail(RA_E_SHAPE, "%s: T=%d (1 .. %d)", who, T, inse::kMaxT);
  if ((long long)Hf * Wf > inse::kMaxPixels || (long long)Hs * Ws >= (1ll << 31) || B > 65535)
    return fail(RA_E_SHAPE, "%s: %dx%d -> %dx%d, B=%d (Hf * Wf <= 2^24, so that every count is exact in float32; Hs * Ws < 2^31; "
                "B <= 65535)", who, Hs, Ws, Hf, Wf, B);
  inse::Thresholds thr;
  inse::Order order;
  if (int rc = inse::prepare(who, B, T, Hs, Ws, thresholds, K, thr, order)) return rc;
  const int vec = Wf % 4 == 0 && (reinterpret_cast<uintptr_t>(gt_ids) & 15) == 0 && (!fg || (reinterpret_cast<uintptr_t>(fg) & 3) == 0);
  return inse::launch_all(who, yc, gt_ids, inst_id, fg, B, T, Hs, Ws, geo::Uniform{Hf, Wf, vec}, inse::grid_x(B, Hf, Wf), morph, thr,
                          order, K, inter, area_b, map, as_stream(stream));
}

int counts_ragged(const char *who, const float *yc, const int *gt_ids, const int *inst_id, const unsigned char *fg, size_t total,
                  const ra_image_geo *geo, ra_image_geo *geo_dev, int B, int T, int Hs, int Ws, int morph, const float *thresholds,
                  int K, int *inter, int *area_b, unsigned short *map, void *stream) {
  if (!yc || !gt_ids || !inst_id || !geo || !geo_dev || !thresholds || !inter || !area_b || B <= 0 || Hs <= 0 || Ws <= 0)
    return fail(RA_E_INVALID, "%s: bad argument", who);
  if ((long long)Hs * Ws >= (1ll << 31) || B > 65535)
    return fail(RA_E_SHAPE, "%s: %dx%d, B=%d (Hs * Ws < 2^31; B <= 65535)", who, Hs, Ws, B);
  inse::Thresholds thr;
  inse::Order order;
  if (int rc = inse::prepare(who, B, T, Hs, Ws, thresholds, K, thr, order)) return rc;
  if (int rc = geo::check(who, geo, B, total, inse::kMaxPixels, "h * w <= 2^24, so that every count is exact in float32")) return rc;
  int ntiles = 0;  // of the largest image: the grid; a workgroup's loop bound is its own image's count
  for (int b = 0; b < B; ++b) ntiles = inse::tiles(geo[b].h, geo[b].w) > ntiles ? inse::tiles(geo[b].h, geo[b].w) : ntiles;
  const int want = inse::kWgs / B > 0 ? inse::kWgs / B : 1;
  hipStream_t st = as_stream(stream);
  if (int rc = geo::upload(who, geo, geo_dev, B, st)) return rc;
  const int vec = (reinterpret_cast<uintptr_t>(gt_ids) & 15) == 0 && (!fg || (reinterpret_cast<uintptr_t>(fg) & 3) == 0);
  return inse::launch_all(who, yc, gt_ids, inst_id, fg, B, T, Hs, Ws, geo::Ragged{geo_dev, vec}, ntiles < want ? ntiles : want, morph,
                          thr, order, K, inter, area_b, map, st);
}

}  // namespace

extern "C" int ra_instance_eval_counts_f32(const float *yc, const int *gt_ids, const int *inst_id, const unsigned char *fg,
                                           int B, int T, int Hs, int Ws, int Hf, int Wf, int morph, const float *thresholds,
                                           int K, int *inter, int *area_b, void *stream) {
  return counts_uniform("ra_instance_eval_counts_f32", yc, gt_ids, inst_id, fg, B, T, Hs, Ws, Hf, Wf, morph, thresholds, K, inter,
                        area_b, nullptr, stream);
}

extern "C" int ra_instance_eval_counts_map_f32(const float *yc, const int *gt_ids, const int *inst_id, const unsigned char *fg,
                                               int B, int T, int Hs, int Ws, int Hf, int Wf, int morph, const float *thresholds,
                                               int K, int *inter, int *area_b, unsigned short *map, void *stream) {
  const char *who = "ra_instance_eval_counts_map_f32";
  if (!map) return fail(RA_E_INVALID, "%s: bad argument", who);
  return counts_uniform(who, yc, gt_ids, inst_id, fg, B, T, Hs, Ws, Hf, Wf, morph, thresholds, K, inter, area_b, map, stream);
}

extern "C" int ra_instance_eval_counts_ragged_f32(const float *yc, const int *gt_ids, const int *inst_id, const unsigned char *fg,
                                                  size_t total, const ra_image_geo *geo, ra_image_geo *geo_dev, int B, int T,
                                                  int Hs, int Ws, int morph, const float *thresholds, int K, int *inter,
                                                  int *area_b, void *stream) {
  return counts_ragged("ra_instance_eval_counts_ragged_f32", yc, gt_ids, inst_id, fg, total, geo, geo_dev, B, T, Hs, Ws, morph,
                       thresholds, K, inter, area_b, nullptr, stream);
}

extern "C" int ra_instance_eval_counts_map_ragged_f32(const float *yc, const int *gt_ids, const int *inst_id,
                                                      const unsigned char *fg, size_t total, const ra_image_geo *geo,
                                                      ra_image_geo *geo_dev, int B, int T, int Hs, int Ws, int morph,
                                                      const float *thresholds, int K, int *inter, int *area_b,
                                                      unsigned short *map, void *stream) {
  const char *who = "ra_instance_eval_counts_map_ragged_f32";
  if (!map) return fail(RA_E_INVALID, "%s: bad argument", who);
  return counts_ragged(who, yc, gt_ids, inst_id, fg, total, geo, geo_dev, B, T, Hs, Ws, morph, thresholds, K, inter, area_b, map,
                       stream);
}

extern "C" int ra_instance_eval_threshold_pos(const float *thresholds, int K, int *pos) {
  const char *who = "ra_instance_eval_threshold_pos";
  if (!thresholds || !pos) return fail(RA_E_INVALID, "%s: bad argument", who);
  inse::Thresholds thr;
  inse::Order order;
  if (int rc = inse::prepare(who, 1, 1, 1, 1, thresholds, K, thr, order)) return rc;
  for (int k = 0; k < K; ++k) pos[k] = order.pos[k];
  return 0;
}
