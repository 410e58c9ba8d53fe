// K16 — evaluating the pre-stage fg_model on the device: what the reference's Evaluator logs while it trains the pre-stage
// (fg_model_train.py:131-133, defined at fg_model.py:196-248) and the whole-dataset foreground / background IoU per threshold
// of fg_model_eval.py:134-178 (analysis.py:834-906).  Both are one memory pass over data that is already on the device.
//
//   stats   ra_fg_stats_f32: the sums behind iou_soft, iou_hard, the (b)ce, orientation_ce and orientation_acc, straight from
//           the logits [npix, nsc + no] and the ground truth at network size.  A thread evaluates the head of one pixel with
//           the expressions of convw::fg_head (ra_conv_wide.hip: 1 / (1 + expf(-x)); expf(v - max) / sum) — unquantised — and
//           adds that pixel's channels in float32 (at most 16 terms for the classes, 8 for the orientation).  Everything after
//           that is float64 in a fixed order: the thread's pixels (a grid-stride walk whose grid depends on npix alone), the
//           wave (xor shuffles), the workgroup's four waves, the workgroups' partials in ws and the finishing launch.  No
//           floating-point atomic anywhere: two runs give the same bits.
//           The HARD quantities are defined on the LOGITS: [logit > 0] for one class, [logit[c] == max_c logit] for several
//           (every maximum counts, as tf.equal does), the first maximum of the orientation logits.  In exact arithmetic that is
//           the reference's y_out > 0.5, y_out == max y_out and argmax(d_out); in float32 two different logits can round to the
//           same probability, and a tie invented by the rounding of a softmax must not count.
//           The channels of a pixel are read element by element at a stride of nsc + no floats (17 for Cityscapes, no vector
//           load fits), the pattern of fg_head; the tensor is 9 MB at 256 x 512 and was written by the layer in front.
//
//   sweep   ra_fg_sweep_counts_f32: v = bilateralFilter(resize(src), 5, 10, 10) evaluated tile by tile and never written.
//           A workgroup owns tiles of kTH x kTW = 16 x 128 full-size pixels.  Phase 1: the resize (ra_resample.h) of the tile
//           plus a 2-pixel halo into LDS, 20 rows of 132 floats; a halo coordinate goes through reflect101 in full-size
//           coordinates first, so LDS holds exactly the values the plane kernel bilateral5_kernel would fetch.  The source
//           plane is small (512 KB at 256 x 512) and stays in L1 / L2.  Phase 2: a thread filters 4 consecutive pixels of two
//           rows; per row it reads its 5 x 8 window as ten ds_read_b128.  The 32 lanes of a tile row read 32 consecutive
//           16-byte slots, so each of the instruction's 16-lane groups touches 16 different slots of the 64 banks: free of
//           conflicts at any row pitch that is a multiple of 4 floats.  Its 4 bytes of gt are ONE 32-bit load when W % 4 == 0
//           and gt is 4-byte aligned — a wave then reads two full 128-byte lines, each byte of gt once — and byte loads
//           otherwise.  The counters are per-lane integers in registers (K padded to 4 or 16 with +inf, so every index is a
//           constant; counting count_a by wave masks in scalar registers instead spilled 294 of them at K = 16), reduced
//           across the wave by shuffles, across the four waves in LDS, and leave the workgroup as ONE 64-bit integer atomic
//           add per counter: integer sums do not depend on the order.  The grid is capped (kSweepWgs workgroups in all) and a workgroup walks several tiles, so the
//           number of atomics does not grow with the image.  ra_fg_sweep_counts_ragged_f32 runs the same kernel over a batch of
//           mixed full sizes: gt flat, image n at its entry of the geometry table (ra_ragged.h), read once per workgroup.
#include <cstdint>

#include "ra_common.h"
#include "ra_ragged.h"
#include "ra_resample.h"

namespace ra {
namespace fge {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------------------------------------------------------- statistics
constexpr int kNS = RA_FG_STAT_COUNT;
constexpr int kStatMaxWgs = 1024;  // four workgroups per CU; the grid is min(ceil(npix / 256), kStatMaxWgs): a function of npix alone
constexpr float kEps = 1e-5f;      // modellib.py:420,426

inline int stat_wgs(size_t npix) {
  const size_t n = (npix + 255) / 256;
  return (int)(n < (size_t)kStatMaxWgs ? n : (size_t)kStatMaxWgs);
}

// the sums of one pixel, float32; l: its nsc + no logits, g: its nsc ground-truth values, dg: its 8 orientation targets
template <bool ORI>
__device__ __forceinline__ void pixel_sums(const float *l, const float *g, const float *dg, int nsc, float (&s)[kNS]) {
  float m;
  if (nsc == 1) {
    const float x = l[0], gg = g[0];
    const float y = 1.f / (1.f + expf(-x));  // fg_head
    const float hard = x > 0.f ? 1.f : 0.f;  // y_out > 0.5 (fg_model.py:209), on the logit
    s[RA_FG_STAT_INTER_SOFT] = y * gg;
    s[RA_FG_STAT_SUM_SOFT] = y;
    s[RA_FG_STAT_SUM_GT] = gg;
    s[RA_FG_STAT_INTER_HARD] = hard * gg;
    s[RA_FG_STAT_SUM_HARD] = hard;
    s[RA_FG_STAT_SEG_CE] = -gg * logf(y + kEps) - (1.f - gg) * logf(1.f - y + kEps);  // f_bce, modellib.py:424-427
    m = gg;  // fg_model.py:205
  } else {
    float v[16], gt[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      v[k] = k < nsc ? l[k] : 0.f;
      gt[k] = k < nsc ? g[k] : 0.f;
    }
    float mx = v[0];
#pragma unroll
    for (int k = 1; k < 16; ++k)
      if (k < nsc) mx = fmaxf(mx, v[k]);
    float e[16], sum = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k)
      if (k < nsc) {
        e[k] = expf(v[k] - mx);  // softmax_n of fg_head: the same expressions in the same order
        sum += e[k];
      }
    float is = 0.f, ss = 0.f, sg = 0.f, ih = 0.f, sh = 0.f, ce = 0.f;
    m = gt[1];
#pragma unroll
    for (int k = 0; k < 16; ++k)
      if (k < nsc) {
        const float y = e[k] / sum;
        ce += -gt[k] * logf(y + kEps);  // f_ce over ALL channels, modellib.py:418-421
        if (k >= 1) {                   // the IoUs leave the background channel out (fg_model.py:215-218)
          const float hard = v[k] == mx ? 1.f : 0.f;  // tf.equal(y_out, max): every maximum counts
          is += y * gt[k];
          ss += y;
          sg += gt[k];
          ih += hard * gt[k];
          sh += hard;
          m = fmaxf(m, gt[k]);  // fg_model.py:202-203
        }
      }
    s[RA_FG_STAT_INTER_SOFT] = is;
    s[RA_FG_STAT_SUM_SOFT] = ss;
    s[RA_FG_STAT_SUM_GT] = sg;
    s[RA_FG_STAT_INTER_HARD] = ih;
    s[RA_FG_STAT_SUM_HARD] = sh;
    s[RA_FG_STAT_SEG_CE] = ce;
  }
  s[RA_FG_STAT_MASK] = ORI ? m : 0.f;
  s[RA_FG_STAT_ORI_CE] = s[RA_FG_STAT_ORI_CORRECT] = 0.f;
  if (ORI) {
    float d[8], t[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      d[k] = l[nsc + k];
      t[k] = dg[k];
    }
    float mx = d[0], tmx = t[0];
    int arg = 0, targ = 0;
#pragma unroll
    for (int k = 1; k < 8; ++k) {
      if (d[k] > mx) mx = d[k], arg = k;      // strict: the first maximum wins (tf.argmax)
      if (t[k] > tmx) tmx = t[k], targ = k;
    }
    float e[8], sum = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      e[k] = expf(d[k] - mx);
      sum += e[k];
    }
    float ce = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) ce += -t[k] * logf(e[k] / sum + kEps);
    s[RA_FG_STAT_ORI_CE] = ce * m;                            // fg_model.py:237-238
    s[RA_FG_STAT_ORI_CORRECT] = (arg == targ ? 1.f : 0.f) * m;  // :242-245
  }
}

template <bool ORI>
__global__ __launch_bounds__(256) void stats_kernel(const float *logits, const float *y_gt, const float *d_gt, size_t npix,
                                                     int nsc, double *part) {
  __shared__ double red[4][kNS];
  const int C = nsc + (ORI ? 8 : 0);
  double acc[kNS];
#pragma unroll
  for (int i = 0; i < kNS; ++i) acc[i] = 0.0;
  for (size_t p = (size_t)blockIdx.x * 256 + threadIdx.x; p < npix; p += (size_t)gridDim.x * 256) {
    float s[kNS];
    pixel_sums<ORI>(logits + p * C, y_gt + p * nsc, ORI ? d_gt + p * 8 : nullptr, nsc, s);
#pragma unroll
    for (int i = 0; i < kNS; ++i) acc[i] += (double)s[i];
  }
#pragma unroll
  for (int i = 0; i < kNS; ++i) {
    double v = acc[i];
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][i] = v;
  }
  __syncthreads();
  if (threadIdx.x < kNS)
    part[(size_t)blockIdx.x * kNS + threadIdx.x] =
        ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

// one workgroup: thread t adds the partials t, t + 256, ... of a slot in that order, a tree in LDS adds the threads
__global__ __launch_bounds__(256) void stats_finish_kernel(const double *part, int nwg, double *out) {
  __shared__ double red[256];
  const int tid = threadIdx.x;
  for (int i = 0; i < kNS; ++i) {
    double a = 0.0;
    for (int w = tid; w < nwg; w += 256) a += part[(size_t)w * kNS + i];
    red[tid] = a;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
      if (tid < off) red[tid] += red[tid + off];
      __syncthreads();
    }
    if (tid == 0) out[i] = red[0];
    __syncthreads();
  }
}

// --------------------------------------------------------------------------------------------------------------------- sweep
constexpr int kMaxK = RA_FG_SWEEP_MAX_K;  // 16
constexpr int kTH = 16, kTW = 128;        // the tile: 256 threads x 2 rows x 4 pixels
constexpr int kLH = kTH + 4, kLW = kTW + 4;  // with the halo of the 5 x 5 window; kLW % 4 == 0 keeps ds_read_b128 aligned
constexpr int kSweepWgs = 1024;           // workgroups in all: four per CU
constexpr int kSlots = RA_FG_SWEEP_SLOTS;  // count_a[16] | sum_ab[16] | sum_b

struct Thresholds {
  float t[kMaxK];
};

__host__ __device__ inline int sweep_tiles_x(int W) { return ceil_div(W, kTW); }
__host__ __device__ inline int sweep_tiles(int H, int W) { return ceil_div(H, kTH) * sweep_tiles_x(W); }
inline int sweep_wgs(int N, int H, int W) {
  const int tiles = sweep_tiles(H, W), want = kSweepWgs / N > 0 ? kSweepWgs / N : 1;
  return tiles < want ? tiles : want;
}

// KP: thresholds compared per pixel (K padded with +inf, which no value exceeds).  VEC: 4 bytes of gt as one 32-bit load.
// GEO: geo::Uniform (gt is [N,H,W]; VEC is the launch's decision) or geo::Ragged (gt flat, image n at its table entry with its
// own H, W; VEC says the base pointer allows it and the image's own vec decides, once per workgroup).
template <int KP, bool VEC, class GEO>
__global__ __launch_bounds__(256) void sweep_kernel(const float *src, const unsigned char *gt, int Hs, int Ws, const GEO geom,
                                                     const Thresholds thr, unsigned long long *counts) {
  __shared__ __attribute__((aligned(16))) float tile[kLH * kLW];
  __shared__ unsigned red[4][2 * KP + 1];
  const int n = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
  const int tx = tid & 31, ty = tid >> 5;  // 4 pixels at column 4 tx of the rows ty and ty + 8
  const float *sp = src + (size_t)n * Hs * Ws;
  const geo::Image im = geom.at(n);
  const int H = im.h, W = im.w;
  const bool vec = VEC && (!GEO::kRagged || im.vec);
  const unsigned char *gp = gt + im.off;
  const float gs = resample::bilateral_gain(10.f), gc = resample::bilateral_gain(10.f);  // fg_model_eval.py:116
  const int ntx = sweep_tiles_x(W), ntiles = sweep_tiles(H, W);
  unsigned cnt_a[KP], sum_ab[KP], sum_b = 0;  // per lane
#pragma unroll
  for (int k = 0; k < KP; ++k) cnt_a[k] = sum_ab[k] = 0;

  for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int r0 = (t / ntx) * kTH, c0 = (t % ntx) * kTW;
    __syncthreads();  // the previous tile's readers are done
    for (int e = tid; e < kLH * kLW; e += 256) {
      const int ly = e / kLW, lx = e - ly * kLW;
      const int r = resample::reflect101(r0 + ly - 2, H), c = resample::reflect101(c0 + lx - 2, W);
      tile[e] = resample::resize_linear_at(sp, Hs, Ws, H, W, r, c);
    }
    __syncthreads();
#pragma unroll 1
    for (int half = 0; half < 2; ++half) {
      const int row = ty + 8 * half, r = r0 + row, c = c0 + 4 * tx;
      unsigned g[4] = {0, 0, 0, 0};
      const bool row_in = r < H;
      if (vec) {
        if (row_in && c < W) {  // W % 4 == 0: c + 3 < W
          const unsigned w = *reinterpret_cast<const unsigned *>(gp + (size_t)r * W + c);
#pragma unroll
          for (int j = 0; j < 4; ++j) g[j] = (w >> (8 * j)) & 255u;
        }
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (row_in && c + j < W) g[j] = gp[(size_t)r * W + c + j];
      }
      f32x4 win[5][2];  // rows row .. row + 4 of LDS, columns 4 tx .. 4 tx + 7: the 5 x 5 windows of the 4 pixels
#pragma unroll
      for (int dy = 0; dy < 5; ++dy) {
        const f32x4 *q = reinterpret_cast<const f32x4 *>(tile + (row + dy) * kLW + 4 * tx);
        win[dy][0] = q[0];
        win[dy][1] = q[1];
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const auto at = [&](int dy, int dx) {
          const int x = j + dx + 2;  // 0 .. 7, a constant after unrolling
          return win[dy + 2][x >> 2][x & 3];
        };
        const float v = resample::bilateral5_at(at, at(0, 0), gs, gc);
        const bool in = row_in && c + j < W;
        sum_b += g[j];  // 0 outside the image
#pragma unroll
        for (int k = 0; k < KP; ++k) {
          const bool hit = in && v > thr.t[k];
          cnt_a[k] += hit ? 1u : 0u;
          sum_ab[k] += hit ? g[j] : 0u;
        }
      }
    }
  }
  // wave: shuffles; workgroup: LDS; then one atomic per counter
#pragma unroll
  for (int k = 0; k < KP; ++k) {
    unsigned u = cnt_a[k], v = sum_ab[k];
    for (int o = 32; o > 0; o >>= 1) {
      u += __shfl_xor(u, o, 64);
      v += __shfl_xor(v, o, 64);
    }
    if (lane == 0) {
      red[tid >> 6][k] = u;
      red[tid >> 6][KP + k] = v;
    }
  }
  {
    unsigned v = sum_b;
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if (lane == 0) red[tid >> 6][2 * KP] = v;
  }
  __syncthreads();
  if (tid < 2 * KP + 1) {
    const unsigned long long s = (unsigned long long)red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
    const int slot = tid < KP ? tid : (tid < 2 * KP ? kMaxK + (tid - KP) : 2 * kMaxK);
    if (s) atomicAdd(counts + (size_t)n * kSlots + slot, s);
  }
}

template <int KP, class GEO>
void launch_sweep(bool vec, dim3 grid, hipStream_t st, const float *src, const unsigned char *gt, int Hs, int Ws, const GEO &geom,
                  const Thresholds &thr, unsigned long long *counts) {
  if (vec)
    hipLaunchKernelGGL((sweep_kernel<KP, true, GEO>), grid, dim3(256), 0, st, src, gt, Hs, Ws, geom, thr, counts);
  else
    hipLaunchKernelGGL((sweep_kernel<KP, false, GEO>), grid, dim3(256), 0, st, src, gt, Hs, Ws, geom, thr, counts);
}

// clear -> sweep on one stream, gx workgroups per image; vec: whether the launch may load 4 bytes of gt at once
template <class GEO>
int sweep_all(const char *who, const float *src, const unsigned char *gt, int N, int Hs, int Ws, const GEO &geom, int gx, bool vec,
              const float *thresholds, int K, unsigned long long *counts, hipStream_t st) {
  Thresholds thr;
  for (int k = 0; k < kMaxK; ++k) thr.t[k] = k < K ? thresholds[k] : __builtin_inff();
  char what[96];
  if (hipMemsetAsync(counts, 0, (size_t)N * kSlots * sizeof(unsigned long long), st) != hipSuccess) {
    snprintf(what, sizeof(what), "%s (clear)", who);
    return launch_status(what);
  }
  const dim3 grid(gx, N);
  if (K <= 4)
    launch_sweep<4>(vec, grid, st, src, gt, Hs, Ws, geom, thr, counts);
  else
    launch_sweep<16>(vec, grid, st, src, gt, Hs, Ws, geom, thr, counts);
  return launch_status(who);
}

}  // namespace fge
}  // namespace ra

using namespace ra;

extern "C" size_t ra_fg_stats_workspace_bytes(size_t npix) {
  return npix ? (size_t)fge::stat_wgs(npix) * fge::kNS * sizeof(double) : 0;
}

extern "C" int ra_fg_stats_f32(const float *logits, const float *y_gt, const float *d_gt, size_t npix, int nsc, int no,
                               void *ws, size_t ws_bytes, double *sums, void *stream) {
  if (!logits || !y_gt || !ws || !sums || npix == 0 || (no && !d_gt)) return fail(RA_E_INVALID, "ra_fg_stats_f32: bad argument");
  if (nsc < 1 || nsc > 16 || (no != 0 && no != 8)) return fail(RA_E_SHAPE, "ra_fg_stats_f32: nsc %d (1 .. 16), no %d (0 | 8)", nsc, no);
  if (ws_bytes < ra_fg_stats_workspace_bytes(npix) || (reinterpret_cast<uintptr_t>(ws) & 7))
    return fail(RA_E_WORKSPACE, "ra_fg_stats_f32: workspace");
  const int nwg = fge::stat_wgs(npix);
  double *part = static_cast<double *>(ws);
  hipStream_t st = as_stream(stream);
  if (no)
    hipLaunchKernelGGL(fge::stats_kernel<true>, dim3(nwg), dim3(256), 0, st, logits, y_gt, d_gt, npix, nsc, part);
  else
    hipLaunchKernelGGL(fge::stats_kernel<false>, dim3(nwg), dim3(256), 0, st, logits, y_gt, d_gt, npix, nsc, part);
  if (int rc = launch_status("ra_fg_stats_f32")) return rc;
  hipLaunchKernelGGL(fge::stats_finish_kernel, dim3(1), dim3(256), 0, st, part, nwg, sums);
  return launch_status("ra_fg_stats_f32 (finish)");
}

extern "C" int ra_fg_sweep_counts_f32(const float *src, const unsigned char *gt, int N, int Hs, int Ws, int H, int W,
                                      const float *thresholds, int K, unsigned long long *counts, void *stream) {
  if (!src || !gt || !thresholds || !counts || N <= 0 || Hs <= 0 || Ws <= 0 || H <= 0 || W <= 0)
    return fail(RA_E_INVALID, "ra_fg_sweep_counts_f32: bad argument");
  if (K < 1 || K > fge::kMaxK) return fail(RA_E_SHAPE, "ra_fg_sweep_counts_f32: K=%d thresholds (1 .. %d)", K, fge::kMaxK);
  if ((long long)H * W >= (1ll << 31) || (long long)Hs * Ws >= (1ll << 31) || N > 65535)
    return fail(RA_E_SHAPE, "ra_fg_sweep_counts_f32: %dx%d -> %dx%d, N=%d (planes below 2^31 pixels, N <= 65535)", Hs, Ws, H, W, N);
  const bool vec = W % 4 == 0 && (reinterpret_cast<uintptr_t>(gt) & 3) == 0;
  return fge::sweep_all("ra_fg_sweep_counts_f32", src, gt, N, Hs, Ws, geo::Uniform{H, W, vec ? 1 : 0}, fge::sweep_wgs(N, H, W), vec,
                        thresholds, K, counts, as_stream(stream));
}

extern "C" int ra_fg_sweep_counts_ragged_f32(const float *src, const unsigned char *gt, size_t total, const ra_image_geo *geo,
                                             ra_image_geo *geo_dev, int N, int Hs, int Ws, const float *thresholds, int K,
                                             unsigned long long *counts, void *stream) {
  const char *who = "ra_fg_sweep_counts_ragged_f32";
  if (!src || !gt || !geo || !geo_dev || !thresholds || !counts || N <= 0 || Hs <= 0 || Ws <= 0)
    return fail(RA_E_INVALID, "%s: bad argument", who);
  if (K < 1 || K > fge::kMaxK) return fail(RA_E_SHAPE, "%s: K=%d thresholds (1 .. %d)", who, K, fge::kMaxK);
  if ((long long)Hs * Ws >= (1ll << 31) || N > 65535)
    return fail(RA_E_SHAPE, "%s: %dx%d, N=%d (planes below 2^31 pixels, N <= 65535)", who, Hs, Ws, N);
  if (int rc = geo::check(who, geo, N, total, (1ll << 31) - 1, "h * w < 2^31")) return rc;
  int ntiles = 0;  // of the largest image: the grid; a workgroup's loop bound is its own image's count
  for (int n = 0; n < N; ++n)
    ntiles = fge::sweep_tiles(geo[n].h, geo[n].w) > ntiles ? fge::sweep_tiles(geo[n].h, geo[n].w) : ntiles;
  const int want = fge::kSweepWgs / N > 0 ? fge::kSweepWgs / N : 1;
  hipStream_t st = as_stream(stream);
  if (int rc = geo::upload(who, geo, geo_dev, N, st)) return rc;
  const bool vec = (reinterpret_cast<uintptr_t>(gt) & 3) == 0;
  return fge::sweep_all(who, src, gt, N, Hs, Ws, geo::Ragged{geo_dev, vec ? 1 : 0}, ntiles < want ? ntiles : want, vec, thresholds, K,
                        counts, st);
}
