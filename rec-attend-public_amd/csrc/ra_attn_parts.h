// The band walk of the direct attention kernels: what the extract kernels (ra_attn_direct.hip) and the resample adjoint
// (ra_attn_train.hip) share.  Workgroup = (one tap j, channel group cg, image b).  The tap's row band (2R+1 rows) x the
// window's columns is read in rounds of 4 KR rows and pages of 256 columns: lane = image column (a wave reads 1 KB runs), wave
// w takes rows w, w+4, ..., every thread keeps KR x 4 independent buffer loads in flight; the four waves' sums meet in LDS
// (stage 1), and each output column contracts its band's columns of that row sum with the column filter (stage 2).
// Device code only, all of it inlined: the pieces change no order of arithmetic.
#pragma once
#include "ra_attn_axis.h"

namespace ra {
namespace attnd {

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// Work items are dealt to the 8 XCDs in contiguous chunks (workgroup id % 8 = XCD): the taps of one image share almost all
// their rows, and those re-reads then hit ONE L2.  False: this workgroup has no item.
__device__ __forceinline__ bool band_item(int n_items, int chunk, int &item) {
  const int slot = blockIdx.x >> 3;
  item = (blockIdx.x & 7) * chunk + slot;
  return slot < chunk && item < n_items;
}

// stage-2 role of a thread: output column oi, its band's columns [bi_lo, bi_hi) dealt to `parts` neighbouring lanes
struct Role {
  int parts, oi, part, bi_lo, bi_hi;
  bool owner;
};
template <int PARTS>  // 0: as many lanes per output column as 256 threads allow (4, 2 or 1)
__device__ __forceinline__ Role stage2_role(const Axis &Ax, int t) {
  Role r;
  r.parts = PARTS ? PARTS : (Ax.F * 4 <= 256) ? 4 : (Ax.F * 2 <= 256) ? 2 : 1;
  r.oi = t / r.parts;
  r.part = t - r.oi * r.parts;
  r.owner = r.oi < Ax.F;
  r.bi_lo = r.bi_hi = 0;
  if (r.owner) Ax.band(r.oi, r.bi_lo, r.bi_hi);
  return r;
}
// the sum over the `parts` lanes of an output column
__device__ __forceinline__ float parts_sum(float v, int parts) {
  if (parts >= 2) v += __shfl_xor(v, 1);
  if (parts >= 4) v += __shfl_xor(v, 2);
  return v;
}
__device__ __forceinline__ f32x4 parts_sum(f32x4 v, int parts) {
  if (parts >= 2) {
#pragma unroll
    for (int c = 0; c < 4; ++c) v[c] += __shfl_xor(v[c], 1);
  }
  if (parts >= 4) {
#pragma unroll
    for (int c = 0; c < 4; ++c) v[c] += __shfl_xor(v[c], 2);
  }
  return v;
}

// One load round: thread (wave wv, lane) reads rows rb + 4k + wv, k < KR, at columns cp + 64p + lane, p < 4.  round_pix:
// the pixel, or -1 for a row beyond the band [.., l1) or a column beyond the window [.., w1); pix_off: its byte offset in
// a buffer of px_bytes per pixel — kOOB (beyond every resource) for -1: that load returns 0 and is not issued.
constexpr int kOOB = 0x7fffffff;
__device__ __forceinline__ int round_pix(int rb, int k, int wv, int cp, int p, int lane, int l1, int w1, int W) {
  const int row = rb + 4 * k + wv, col = cp + 64 * p + lane;
  return (row < l1 && col < w1) ? row * W + col : -1;
}
__device__ __forceinline__ int pix_off(int pix, int px_bytes) { return pix >= 0 ? pix * px_bytes : kOOB; }

// The row filter's weights of a round are evaluated once per wave, one per lane — lane k evaluates row rowl = rb + 4k + wv of
// tap j, zero beyond the band's last row — and handed to the multiply-adds through v_readlane (a v_exp costs 16 cycles of
// a SIMD that holds one or two waves).
template <int KR>
__device__ __forceinline__ float row_weight(const Axis &Ay, int j, int rowl, int lane, int l1) {
  return (lane < KR && rowl < l1) ? Ay.w((float)rowl, j) : 0.0f;
}

// stage 1: the four waves' sums of ND row filters over one column page -> red[d][0][t] = column t of the page
template <int ND, typename V>
__device__ __forceinline__ void reduce_waves(V (&red)[ND][4][256], const V (&acc)[ND][4], int t, int wv, int lane) {
  __syncthreads();  // the previous column page's stage 2 is done with `red`
#pragma unroll
  for (int d = 0; d < ND; ++d)
#pragma unroll
    for (int p = 0; p < 4; ++p) red[d][wv][64 * p + lane] = acc[d][p];
  __syncthreads();
#pragma unroll
  for (int d = 0; d < ND; ++d) red[d][0][t] = (red[d][0][t] + red[d][1][t]) + (red[d][2][t] + red[d][3][t]);
  __syncthreads();
}

// stage 2 of the extract contracts red[d][0][..] with the column filter.  This thread's first kPre column-filter weights (terms
// bi_lo + part + u * parts) depend on the record only: the caller evaluates them under the loads' latency, instead of behind
// their wait.  The contraction itself is written in the one kernel body that has it: as a function of this header it cost
// extract_rows_kernel<1, 4> 25 VGPRs and an occupancy step (the same IR in another block order).
constexpr int kPre = 8;
__device__ __forceinline__ void col_weights(const Axis &Ax, const Role &r, float (&fpre)[kPre]) {
#pragma unroll
  for (int u = 0; u < kPre; ++u) {
    const int ww = r.bi_lo + r.part + u * r.parts;
    fpre[u] = (r.owner && ww < r.bi_hi) ? Ax.w((float)ww, r.oi) : 0.0f;
  }
}

}  // namespace attnd
}  // namespace ra
