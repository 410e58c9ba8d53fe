// K19 — training the pre-stage fg_model: the gradient of its loss head (fg_model.py:196-248) with respect to the logits, and
// tf.train.MomentumOptimizer on the flat parameter bucket (fg_model.py:262-263).  The forward value of the loss is
// ra_fg_stats_f32 (ra_fg_eval.hip), unchanged: this file reads the nine sums it left on the device.
//
//   bwd       ra_fg_loss_bwd_f32: dL/dlogits [npix, nsc + no].  The layer is bandwidth-bound — 2 (nsc + no) floats read and
//             nsc + no written per pixel, a few dozen flops — and a pixel's run of C = nsc + no floats (1, 9, 11, 17 in the
//             run scripts) is no multiple of 16 bytes, so a thread that walked its own pixel in global memory would issue C
//             scalar loads at a stride of C floats.  Instead a workgroup owns a tile of 256 consecutive pixels, which is ONE
//             contiguous run of 256 C floats in each tensor, starting at a multiple of 1 KB: the 256 threads copy it into LDS
//             with 16-byte loads of consecutive addresses (a wave reads 1 KB per instruction), each thread then takes its
//             pixel's channels out of LDS into registers, evaluates the adjoint, writes dz back over its logits in LDS, and
//             the tile leaves through 16-byte stores the same way.  The LDS row pitch is C | 1 floats: odd, so the 64 lanes of
//             a wave, reading channel k of 64 consecutive pixels, touch 64 different banks whatever C is.  The last tile is
//             ragged: its run is cut at (npix - p0) C floats, 16-byte pieces up to the last whole one, single floats after.
//             A base pointer that is not 16-byte aligned takes single floats throughout (vec = 0).
//             The head's probabilities are evaluated with the expressions of convw::fg_head and fge::pixel_sums
//             (1 / (1 + expf(-x)); expf(v - max) / sum in channel order), so forward and backward see the same p.
//             The batch-wide terms (1 / U, I / U^2 of the soft IoU, 1 / MASK of the orientation loss) are formed in float64
//             from the sums by every thread — a handful of operations on uniform values — and rounded to float32 once.
//             Nothing is accumulated across threads: no atomics, the same bits on every run.
//   momentum  ra_momentum_step_guarded_f32: one pass over four arrays, the guard of ra_adam_step_guarded_f32.
#include <cstdint>

#include "ra_common.h"

namespace ra {
namespace fgl {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kTile = 256;        // pixels per workgroup, one per thread
constexpr int kMaxSc = 16;        // semantic classes
constexpr int kNo = 8;            // orientation classes
constexpr float kEps = 1e-5f;     // modellib.py:420,426: inside the logarithms, so the derivative is of log(p + eps)
constexpr double kIouEps = 1e-5;  // modellib.py:171-181

// floats of LDS a workgroup needs: logits, y_gt and d_gt tiles at row pitches (nsc + no) | 1, nsc | 1 and 9; at most 51 KB
inline int lds_floats(int nsc, int no) { return kTile * (((nsc + no) | 1) + (nsc | 1) + (no ? kNo + 1 : 0)); }

// tile run src[0 .. n) (n = pixels * C floats) -> LDS rows of `pitch` floats
__device__ __forceinline__ void tile_in(const float *src, int n, int C, int pitch, float *dst, int vec) {
  const int tid = threadIdx.x;
  const int n4 = vec ? n >> 2 : 0;
  const f32x4 *s4 = reinterpret_cast<const f32x4 *>(src);
  for (int i = tid; i < n4; i += kTile) {
    const f32x4 v = s4[i];
    int pix = (4 * i) / C, ch = 4 * i - pix * C;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      dst[pix * pitch + ch] = v[e];
      if (++ch == C) ch = 0, ++pix;
    }
  }
  for (int i = 4 * n4 + tid; i < n; i += kTile) {
    const int pix = i / C;
    dst[pix * pitch + (i - pix * C)] = src[i];
  }
}

__device__ __forceinline__ void tile_out(const float *src, int n, int C, int pitch, float *dst, int vec) {
  const int tid = threadIdx.x;
  const int n4 = vec ? n >> 2 : 0;
  f32x4 *d4 = reinterpret_cast<f32x4 *>(dst);
  for (int i = tid; i < n4; i += kTile) {
    f32x4 v;
    int pix = (4 * i) / C, ch = 4 * i - pix * C;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      v[e] = src[pix * pitch + ch];
      if (++ch == C) ch = 0, ++pix;
    }
    d4[i] = v;
  }
  for (int i = 4 * n4 + tid; i < n; i += kTile) {
    const int pix = i / C;
    dst[i] = src[pix * pitch + (i - pix * C)];
  }
}

// SEG: 0 = iou (loss = -I / U over the whole batch), 1 = (b)ce / num_pixel
template <bool ORI>
__global__ __launch_bounds__(kTile) void loss_bwd_kernel(const float *logits, const float *y_gt, const float *d_gt, size_t npix,
                                                         int nsc, int seg, const double *sums, float upstream, float *dlogits,
                                                         int *status, int vec) {
  extern __shared__ float smem[];  // lds_floats(nsc, no): the three tiles at their own pitches, 19 KB at 1 + 8 classes
  const int C = nsc + (ORI ? kNo : 0), pl = C | 1, py = nsc | 1, pd = kNo + 1;
  float *sl = smem, *sy = sl + kTile * pl, *sd = sy + kTile * py;
  const size_t p0 = (size_t)blockIdx.x * kTile;
  const int np = npix - p0 < (size_t)kTile ? (int)(npix - p0) : kTile;  // pixels of this tile
  tile_in(logits + p0 * C, np * C, C, pl, sl, vec & 1);
  tile_in(y_gt + p0 * nsc, np * nsc, nsc, py, sy, vec & 2);
  if (ORI) tile_in(d_gt + p0 * kNo, np * kNo, kNo, pd, sd, vec & 4);

  // the batch-wide terms, float64 -> float32 once
  const double I = sums[RA_FG_STAT_INTER_SOFT];
  const double U = sums[RA_FG_STAT_SUM_SOFT] + sums[RA_FG_STAT_SUM_GT] - I + kIouEps;
  const float inv_u = (float)(1.0 / U), i_u2 = (float)(I / (U * U));
  const float inv_n = (float)(1.0 / (double)npix);  // num_pixel, fg_model.py:196-199
  const double mask = ORI ? sums[RA_FG_STAT_MASK] : 1.0;
  const bool no_fg = ORI && !(mask > 0.0);
  const float inv_mask = no_fg ? 0.f : (float)(1.0 / mask);
  if (blockIdx.x == 0 && threadIdx.x == 0) status[0] = no_fg ? 1 : 0;
  __syncthreads();

  const int t = threadIdx.x;
  if (t < np) {
    float *l = sl + t * pl;
    const float *g = sy + t * py;
    float m;
    if (nsc == 1) {
      const float x = l[0], gg = g[0];
      const float p = 1.f / (1.f + expf(-x));  // fg_head
      const float q = seg ? (-gg / (p + kEps) + (1.f - gg) / (1.f - p + kEps)) * inv_n : -(gg * inv_u - i_u2 * (1.f - gg));
      l[0] = upstream * q * (p * (1.f - p));
      m = gg;
    } else {
      float v[kMaxSc], gt[kMaxSc], e[kMaxSc];
#pragma unroll
      for (int k = 0; k < kMaxSc; ++k) {
        v[k] = k < nsc ? l[k] : 0.f;
        gt[k] = k < nsc ? g[k] : 0.f;
      }
      float mx = v[0];
#pragma unroll
      for (int k = 1; k < kMaxSc; ++k)
        if (k < nsc) mx = fmaxf(mx, v[k]);
      float sum = 0.f;
#pragma unroll
      for (int k = 0; k < kMaxSc; ++k)
        if (k < nsc) {
          e[k] = expf(v[k] - mx);  // softmax_n of fg_head: the same expressions in the same order
          sum += e[k];
        }
      float dot = 0.f;
      m = gt[1];
#pragma unroll
      for (int k = 0; k < kMaxSc; ++k)
        if (k < nsc) {
          const float p = e[k] / sum;
          float q;
          if (seg) q = -gt[k] / (p + kEps) * inv_n;                        // f_ce over ALL channels (fg_model.py:225)
          else q = k >= 1 ? -(gt[k] * inv_u - i_u2 * (1.f - gt[k])) : 0.f;  // the IoU leaves the background out (:215)
          if (k >= 1) m = fmaxf(m, gt[k]);                                 // :202-203
          e[k] = p;
          v[k] = q;
          dot += p * q;
        }
#pragma unroll
      for (int k = 0; k < kMaxSc; ++k)
        if (k < nsc) l[k] = upstream * (e[k] * (v[k] - dot));  // the softmax adjoint
    }
    if (ORI) {
      const float *tg = sd + t * pd;
      float d[kNo], q[kNo];
#pragma unroll
      for (int k = 0; k < kNo; ++k) d[k] = l[nsc + k];
      float mx = d[0];
#pragma unroll
      for (int k = 1; k < kNo; ++k) mx = fmaxf(mx, d[k]);
      float sum = 0.f;
#pragma unroll
      for (int k = 0; k < kNo; ++k) {
        d[k] = expf(d[k] - mx);
        sum += d[k];
      }
      float dot = 0.f;
#pragma unroll
      for (int k = 0; k < kNo; ++k) {
        d[k] = d[k] / sum;
        q[k] = -tg[k] * m / (d[k] + kEps) * inv_mask;  // fg_model.py:237-239
        dot += d[k] * q[k];
      }
#pragma unroll
      for (int k = 0; k < kNo; ++k) l[nsc + k] = no_fg ? 0.f : upstream * (d[k] * (q[k] - dot));
    }
  }
  __syncthreads();
  tile_out(sl, np * C, C, pl, dlogits + p0 * C, vec & 8);
}

__global__ __launch_bounds__(256) void momentum_kernel(float *p, const float *g, float *acc, const float *wd, size_t n, float lr,
                                                       float momentum, float gscale, const int *status, int n_status) {
  // the guard of train::adam_kernel: any non-zero word of this step (uniform across the grid, written by launches earlier on
  // the stream) and parameters and accumulators stay as they are
  for (int k = 0; k < n_status; ++k)
    if (status[k] != 0) return;
  const size_t stride = (size_t)gridDim.x * 256;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
    const float pi = p[i];
    const float gi = g[i] * gscale + (wd ? wd[i] * pi : 0.f);
    const float ai = momentum * acc[i] + gi;
    acc[i] = ai;
    p[i] = pi - lr * ai;
  }
}

}  // namespace fgl
}  // namespace ra

using namespace ra;

extern "C" int ra_fg_loss_bwd_f32(const float *logits, const float *y_gt, const float *d_gt, size_t npix, int nsc, int no,
                                  int segm_loss_fn, const double *sums, float upstream, float *dlogits, int *status,
                                  void *stream) {
  if (!logits || !y_gt || !sums || !dlogits || !status || npix == 0 || (no && !d_gt))
    return fail(RA_E_INVALID, "ra_fg_loss_bwd_f32: bad argument");
  if (nsc < 1 || nsc > fgl::kMaxSc || (no != 0 && no != fgl::kNo))
    return fail(RA_E_SHAPE, "ra_fg_loss_bwd_f32: nsc %d (1 .. 16), no %d (0 | 8)", nsc, no);
  if (segm_loss_fn != 0 && segm_loss_fn != 1) return fail(RA_E_SHAPE, "ra_fg_loss_bwd_f32: segm_loss_fn %d (0 = iou, 1 = bce)", segm_loss_fn);
  const size_t nwg = (npix + fgl::kTile - 1) / fgl::kTile;
  if (nwg > 0x7fffffffull) return fail(RA_E_SHAPE, "ra_fg_loss_bwd_f32: %zu pixels", npix);
  auto al = [](const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
  const int vec = (al(logits) ? 1 : 0) | (al(y_gt) ? 2 : 0) | (no && al(d_gt) ? 4 : 0) | (al(dlogits) ? 8 : 0);
  hipStream_t st = as_stream(stream);
  const size_t lds = (size_t)fgl::lds_floats(nsc, no) * sizeof(float);
  if (no)
    hipLaunchKernelGGL(fgl::loss_bwd_kernel<true>, dim3((unsigned)nwg), dim3(fgl::kTile), lds, st, logits, y_gt, d_gt, npix, nsc,
                       segm_loss_fn, sums, upstream, dlogits, status, vec);
  else
    hipLaunchKernelGGL(fgl::loss_bwd_kernel<false>, dim3((unsigned)nwg), dim3(fgl::kTile), lds, st, logits, y_gt, d_gt, npix, nsc,
                       segm_loss_fn, sums, upstream, dlogits, status, vec);
  return launch_status("ra_fg_loss_bwd_f32");
}

extern "C" int ra_momentum_step_guarded_f32(float *params, const float *grads, float *accum, const float *wd_coef, size_t n,
                                            float lr, float momentum, float grad_scale, const int *status, int n_status,
                                            void *stream) {
  if (!params || !grads || !accum) return fail(RA_E_INVALID, "ra_momentum_step_guarded_f32: null pointer");
  if (n_status < 0 || (n_status > 0 && !status)) return fail(RA_E_INVALID, "ra_momentum_step_guarded_f32: status words");
  if (n == 0) return 0;
  size_t grid = (n + 255) / 256;
  if (grid > 2048) grid = 2048;
  hipLaunchKernelGGL(fgl::momentum_kernel, dim3((unsigned)grid), dim3(256), 0, as_stream(stream), params, grads, accum, wd_coef, n,
                     lr, momentum, grad_scale, status, n_status);
  return launch_status("ra_momentum_step_guarded_f32");
}
