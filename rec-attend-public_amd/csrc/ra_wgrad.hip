// =================================================================================================
// conv3x3 backward-weight on f32 MFMA.  For the SAME conv u = conv(X, Wf) the kernel returns
//   dWf[ky][kx][ci][co] = sum_{b,y,x} X[b, y+ky-1, x+kx-1, ci] * dU[b, y, x, co]      (X zero-padded;
//   with `upsample` X is the zero-stuffed image of a stride-2 transposed conv) and  db[co] = sum dU.
// GEMM view per tap: D[ci, co] = sum_pixels A[ci, pixel] * B[pixel, co]  — pixels are the K
// dimension of v_mfma_f32_16x16x4_f32 (A = 16 input channels x 4 pixels, B = 4 pixels x 16 couts).
// A workgroup owns a 16-channel slice of Cin (blockIdx.y) and walks 8 x 32 pixel tiles
// persistently; its 4 waves split the tile's rows (K split), every wave keeps all
// 10 (9 taps + bias) x CoutP/16 accumulator tiles for its rows in registers across tiles; at the
// end the waves are summed through LDS and the workgroup writes ONE partial; a second kernel adds
// the partials in a fixed order (deterministic, no atomics).
#include <type_traits>

#include "ra_common.h"

namespace ra {
namespace train {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2q __attribute__((ext_vector_type(2)));

constexpr int WTH = 8, WTW = 32, WLW = WTW + 2, WLH = WTH + 2;

// PACK = 0: the M rows of an MFMA are the 16 input channels of the slice, one accumulator tile per tap
// (9 + bias).  PACK = Cin (4 or 8): the M rows are (tap, channel) pairs, 9 * Cin of them in
// ceil(9 * Cin / 16) tiles — 3 instead of 9 k-step MFMAs per pixel quad for Cin = 4 (where 12 of the 16
// channel rows were zero), 5 for Cin = 8; a lane reads its row's pixel through a per-tile LDS offset.
// BF16 (compute_dtype = 'bf16'): the staged float32 pixels are rounded to bf16 as they leave LDS and four K steps
// (32 consecutive pixels of a row) go through ONE v_mfma_f32_16x16x32_bf16 (the gfx950 form); accumulation stays float32.
typedef short bf16x4 __attribute__((ext_vector_type(4)));
__device__ inline bf16x4 pack_bf16(float v0, float v1, float v2, float v3) {
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
  typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
  const unsigned lo = __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{v0, v1}, bf16x2));
  const unsigned hi = __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{v2, v3}, bf16x2));
  return __builtin_bit_cast(bf16x4, u32x2{lo, hi});
}

// PRE (Cout % 4 == 0, NT <= 2): the NEXT tile's global loads are issued into registers before the MFMA loop of the
// current one and written to LDS after it (one staging buffer, two barriers per tile as before): the loads' latency
// and the HBM stream hide behind the matrix work instead of in front of it.
// four consecutive elements at element offset `off` of a tensor stored as float32 or (bf: the bf16 mode's storage) bf16
__device__ inline f32x4 ld4_fmt(const float *base, size_t off, bool bf) {
  if (bf) {
    const u32x2q q = *reinterpret_cast<const u32x2q *>(reinterpret_cast<const char *>(base) + off * 2);
    return f32x4{__builtin_bit_cast(float, q.x << 16), __builtin_bit_cast(float, q.x & 0xffff0000u),
                 __builtin_bit_cast(float, q.y << 16), __builtin_bit_cast(float, q.y & 0xffff0000u)};
  }
  return *reinterpret_cast<const f32x4 *>(base + off);
}

__device__ inline float ld1_fmt(const float *base, size_t off, bool bf) {
  if (bf) return __builtin_bit_cast(float, (unsigned)reinterpret_cast<const unsigned short *>(base)[off] << 16);
  return base[off];
}

// ---- what the 8-output-channel kernel families share.  wgrad_kernel keeps its own inline copies of the tile location and the
// slot rule: written through these helpers its 26 instantiations compile to other code, and the prefetching 16 -> 16 form
// measured 3.6 % slower (profiles/wgrad_forms.txt) ----
// A tile of the persistent walk: its image b within its segment, the image coordinates of its first pixel, and the segment's
// tensors.  With xtab / dutab the images of several calls of the layer (one per timestep) are walked as one batch: segment
// tables, Bseg images each.
template <typename P>
struct WTile { int b, ty0, tx0; P x, du; };
template <typename P>
__device__ inline WTile<P> locate_tile(int tile, int per, int tiles_x, P x, P du, P const *xtab, P const *dutab, int Bseg) {
  int b = tile / per;
  const int tr = tile - b * per;
  P ub = du, xb = x;
  if (xtab) {
    const int seg = b / Bseg;
    xb = xtab[seg];
    ub = dutab[seg];
    b -= seg * Bseg;
  }
  return {b, (tr / tiles_x) * WTH, (tr % tiles_x) * WTW, xb, ub};
}

// Partial record of a workgroup: [tap (9 = bias)][channel of the 16-channel slice][CP].  Row R of the (tap, ci) rows packed
// CIN per tap, the bias row last (R = 9 CIN) -> its slot tap * 16 + ci of the record; -1 = a padding row.
template <int CIN>
__device__ inline int row_slot(int R) {
  if (R < 9 * CIN) {
    const int tap = R / CIN;
    return tap * 16 + (R - tap * CIN);
  }
  return R == 9 * CIN ? 9 * 16 : -1;
}
constexpr int record_floats(int CP) { return 10 * 16 * CP; }

// The four waves of a workgroup saw different pixels: each puts its sums into its own zeroed copy of the record in LDS
// (put(copy): slots it does not write stay zero), and the copies are added in the fixed order (0 + 1) + (2 + 3) into dst.
template <typename F>
__device__ inline void sum_wave_records(float *red, int CP, float *dst, F &&put) {  // red: [wave][tap (9 = bias)][16][CP]
  const int tid = threadIdx.x, rec = record_floats(CP);
  for (int e = tid; e < 4 * rec; e += 256) red[e] = 0.f;
  __syncthreads();
  put(red + (tid >> 6) * rec);
  __syncthreads();
  for (int e = tid; e < rec; e += 256) dst[e] = (red[e] + red[e + rec]) + (red[e + 2 * rec] + red[e + 3 * rec]);
}

// Dynamic LDS of each form in bytes, for its kernel and its launch: the staged tile(s), or the record(s) that reuse the space
constexpr size_t max_bytes(size_t a, size_t b) { return a > b ? a : b; }
// wgrad_kernel: x slice + halo [WLH][WLW][16], dU tile [WTH][WTW][CP], then ONE record; wgrad_small_kernel: [WLH][WLW][CIN + 1],
// [WTH][WTW][9], then the four waves' records
constexpr size_t generic_lds_bytes(int CP) { return max_bytes((WLH * WLW * 16 + WTH * WTW * CP) * 4, record_floats(CP) * 4); }
constexpr size_t block16_lds_bytes(int CIN, int CP) { return max_bytes((WLH * WLW * (CIN + 1) + WTH * WTW * 9) * 4, 4 * record_floats(CP) * 4); }
// the DMA forms: tiles of 16-byte items, pixel-major as they lie in memory, the x tile in whole 64-lane pieces; two buffers
constexpr int dma_x_bytes(int xpb) { return (WLH * WLW * (xpb / 16) + 63) / 64 * 1024; }
constexpr int dma_u_bytes(int upb) { return WTH * WTW * upb; }
constexpr size_t dma_lds_bytes(int xpb, int upb, int CP) { return max_bytes(2 * (dma_x_bytes(xpb) + dma_u_bytes(upb)), 4 * record_floats(CP) * 4); }

template <int NT, int PACK = 0, bool BF16 = false, bool PRE = false>  // NT: output channels per workgroup / 16; blockIdx.z selects a 16*NT-wide slice of Cout
__global__ __launch_bounds__(256) void wgrad_kernel(const float *x, const float *du, int B, int Hs, int Ws, int Cin,
                                                    int ups, int H, int W, int Cout, int tiles_x, int tiles_y,
                                                    int ntiles, float *part, const float *const *xtab,
                                                    const float *const *dutab, int Bseg, int fmt) {
  // fmt (BF16 kernels only): bit 0 = x is stored as bf16, bit 1 = du is stored as bf16
  const bool xbf = BF16 && (fmt & 1), ubf = BF16 && (fmt & 2);
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float *tx = lds;                      // [WLH][WLW][16]   input slice + halo, channel-contiguous
  float *tu = lds + WLH * WLW * 16;     // [WTH][WTW][16*NT] output gradient tile
  constexpr int CP = 16 * NT;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m = lane & 15, ksub = lane >> 4;
  const int co0 = blockIdx.z * 16 * NT;       // first output channel of this workgroup's slice
  const int c0 = blockIdx.y * 16;             // first input channel of this workgroup's slice
  const int cn = Cin - c0 < 16 ? Cin - c0 : 16;  // real channels in the slice
  constexpr int MT = PACK ? (9 * PACK + 15) / 16 : 9;  // accumulator tiles of the filter taps; tile MT = the bias
  f32x4 acc[MT + 1][NT];
#pragma unroll
  for (int t = 0; t <= MT; ++t)
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[t][n] = f32x4{0.f, 0.f, 0.f, 0.f};
  // PACK: LDS offset (floats, relative to the lane's pixel) of row m of tile t: its tap's pixel shift + its
  // channel; padding rows read channel 15 of the pixel, which is staged as zero (cn <= 8)
  int aoff[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    if constexpr (PACK != 0) {
      const int R = 16 * t + m, tap = R / PACK, ci = R - tap * PACK;
      aoff[t] = tap < 9 ? ((tap / 3) * WLW + tap % 3) * 16 + ci : 15;
    } else {
      aoff[t] = ((t / 3) * WLW + t % 3) * 16 + m;
    }
  }
  // the channel groups beyond the slice's real channels are zero for the whole launch: written once, not per tile
  const int ng = (cn + 3) >> 2;
  if (ng < 4) {
    for (int e = tid; e < WLH * WLW * 4; e += 256) *reinterpret_cast<f32x4 *>(tx + e * 4) = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  const bool vec_du = (Cout & 3) == 0;  // float4 loads of the output gradient
  const int per = tiles_x * tiles_y;
  constexpr int NRX = PRE ? (WLH * WLW * 4 + 255) / 256 : 1, NRU = PRE ? CP / 4 : 1;
  f32x4 rx[NRX], ru[NRU];
  auto prefetch = [&](int tile) {  // every load unconditional (clamped address, value selected afterwards)
    int b = tile / per;
    const int tr = tile - b * per;
    const float *xb = x, *ub = du;
    if (xtab) {
      const int seg = b / Bseg;
      xb = xtab[seg];
      ub = dutab[seg];
      b -= seg * Bseg;
    }
    const int ty0 = (tr / tiles_x) * WTH, tx0 = (tr % tiles_x) * WTW;
    auto load_x = [&](auto bf) {  // the storage format is uniform: ONE test around the whole unrolled loop
#pragma unroll
      for (int i = 0; i < NRX; ++i) {
        const int e = tid + 256 * i;
        const int pix = e / ng, c4 = e - pix * ng;
        const int r = pix / WLW, c = pix - r * WLW;
        const int Y = ty0 + r - 1, X = tx0 + c - 1;
        bool ok = (e < WLH * WLW * ng) & (Y >= 0) & (Y < H) & (X >= 0) & (X < W);
        int ys = Y, xs = X;
        if (ups) {
          ok = ok & (Y & 1) & (X & 1);
          ys = (Y - 1) >> 1;
          xs = (X - 1) >> 1;
        }
        const size_t off = ok ? (((size_t)b * Hs + ys) * Ws + xs) * Cin + c0 + 4 * c4 : 0;
        const f32x4 v = ld4_fmt(xb, off, decltype(bf)::value);
        rx[i] = ok ? v : f32x4{0.f, 0.f, 0.f, 0.f};
      }
    };
    auto load_u = [&](auto bf) {
#pragma unroll
      for (int i = 0; i < NRU; ++i) {
        const int e = tid + 256 * i;
        const int c4 = e % (CP / 4), pix = e / (CP / 4);
        const int r = pix / WTW, c = pix - r * WTW;
        const int Y = ty0 + r, X = tx0 + c;
        const bool ok = (Y < H) & (X < W) & (co0 + 4 * c4 < Cout);
        const size_t off = ok ? (((size_t)b * H + Y) * W + X) * Cout + co0 + 4 * c4 : 0;
        const f32x4 v = ld4_fmt(ub, off, decltype(bf)::value);
        ru[i] = ok ? v : f32x4{0.f, 0.f, 0.f, 0.f};
      }
    };
    if (xbf) load_x(std::true_type{}); else load_x(std::false_type{});
    if (ubf) load_u(std::true_type{}); else load_u(std::false_type{});
  };
  auto commit = [&]() {  // the prefetched tile -> LDS
#pragma unroll
    for (int i = 0; i < NRX; ++i) {
      const int e = tid + 256 * i;
      const int pix = e / ng, c4 = e - pix * ng;
      if (e < WLH * WLW * ng) *reinterpret_cast<f32x4 *>(tx + pix * 16 + 4 * c4) = rx[i];
    }
#pragma unroll
    for (int i = 0; i < NRU; ++i) {
      const int e = tid + 256 * i;
      const int c4 = e % (CP / 4), pix = e / (CP / 4);
      *reinterpret_cast<f32x4 *>(tu + pix * CP + 4 * c4) = ru[i];
    }
  };
  if constexpr (PRE) {
    if ((int)blockIdx.x < ntiles) prefetch(blockIdx.x);
  }
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    int b = tile / per;
    const int tr = tile - b * per;
    if (xtab) {  // the images of several calls of the layer (one per timestep): segment tables, Bseg images each
      const int seg = b / Bseg;
      x = xtab[seg];
      du = dutab[seg];
      b -= seg * Bseg;
    }
    const int ty0 = (tr / tiles_x) * WTH, tx0 = (tr % tiles_x) * WTW;
    __syncthreads();  // the previous tile's MFMA reads are complete
    if constexpr (PRE) {
      commit();
      __syncthreads();
      if (tile + (int)gridDim.x < ntiles) prefetch(tile + gridDim.x);  // in flight across the MFMA loop below
    } else {
    for (int e = tid; e < WLH * WLW * ng; e += 256) {  // input slice: one float4 (4 channels) per item
      const int pix = e / ng, c4 = e - pix * ng;
      const int r = pix / WLW, c = pix - r * WLW;
      const int Y = ty0 + r - 1, X = tx0 + c - 1;
      bool ok = (Y >= 0) & (Y < H) & (X >= 0) & (X < W);
      int ys = Y, xs = X;
      if (ups) {
        ok = ok & (Y & 1) & (X & 1);
        ys = (Y - 1) >> 1;
        xs = (X - 1) >> 1;
      }
      f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
      if (ok) v = ld4_fmt(x, (((size_t)b * Hs + ys) * Ws + xs) * Cin + c0 + 4 * c4, xbf);
      *reinterpret_cast<f32x4 *>(tx + pix * 16 + 4 * c4) = v;
    }
    if (vec_du) {
      for (int e = tid; e < WTH * WTW * (CP / 4); e += 256) {  // output-gradient tile, zero beyond Cout / the image
        const int c4 = e % (CP / 4), pix = e / (CP / 4);
        const int r = pix / WTW, c = pix - r * WTW;
        const int Y = ty0 + r, X = tx0 + c;
        f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
        if (Y < H && X < W && co0 + 4 * c4 < Cout)
          v = ld4_fmt(du, (((size_t)b * H + Y) * W + X) * Cout + co0 + 4 * c4, ubf);
        *reinterpret_cast<f32x4 *>(tu + pix * CP + 4 * c4) = v;
      }
    } else {
      for (int e = tid; e < WTH * WTW * CP; e += 256) {
        const int co = e % CP, pix = e / CP;
        const int r = pix / WTW, c = pix - r * WTW;
        const int Y = ty0 + r, X = tx0 + c;
        float v = 0.f;
        if (Y < H && X < W && co0 + co < Cout) v = ld1_fmt(du, (((size_t)b * H + Y) * W + X) * Cout + co0 + co, ubf);
        tu[e] = v;
      }
    }
    __syncthreads();
    }
    // this wave's rows: 2 of the 8; K steps of 4 consecutive pixels of a row
#pragma unroll 1
    for (int rr = 0; rr < 2; ++rr) {
      const int row = wave * 2 + rr;
      if constexpr (BF16) {
        // v_mfma_f32_16x16x32_bf16 (gfx950): a lane's 8 k-values = its pixels col, col + 4, ..., col + 28 of the row (two of
        // the K = 16 form's quads; slot j of the A lane meets slot j of the B lane, so any shared assignment contracts right)
        static_assert(WTW % 32 == 0, "32 pixels of a row per MFMA");
        typedef short bf16x8s __attribute__((ext_vector_type(8)));
        typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
        auto cat8 = [](bf16x4 lo, bf16x4 hi) { return __builtin_bit_cast(bf16x8, (bf16x8s)__builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7)); };
#pragma unroll
        for (int s0 = 0; s0 < WTW / 32; ++s0) {
          const int col = 32 * s0 + ksub;
          bf16x8 bv[NT];
#pragma unroll
          for (int n = 0; n < NT; ++n) {
            const float *q = tu + (row * WTW + col) * CP + 16 * n + m;
            bv[n] = cat8(pack_bf16(q[0], q[4 * CP], q[8 * CP], q[12 * CP]), pack_bf16(q[16 * CP], q[20 * CP], q[24 * CP], q[28 * CP]));
          }
#pragma unroll
          for (int t = 0; t < MT; ++t) {
            const float *q = tx + (row * WLW + col) * 16 + aoff[t];
            const bf16x8 av = cat8(pack_bf16(q[0], q[64], q[128], q[192]), pack_bf16(q[256], q[320], q[384], q[448]));
#pragma unroll
            for (int n = 0; n < NT; ++n) acc[t][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, bv[n], acc[t][n], 0, 0, 0);
          }
          const bf16x4 one4 = bf16x4{0x3F80, 0x3F80, 0x3F80, 0x3F80};
          const bf16x8 one = cat8(one4, one4);
#pragma unroll
          for (int n = 0; n < NT; ++n) acc[MT][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(one, bv[n], acc[MT][n], 0, 0, 0);
        }
        continue;
      }
#pragma unroll 2
      for (int s = 0; s < WTW / 4; ++s) {
        const int col = 4 * s + ksub;  // this lane's pixel within the K step
        float bv[NT];
#pragma unroll
        for (int n = 0; n < NT; ++n) bv[n] = tu[(row * WTW + col) * CP + 16 * n + m];
#pragma unroll
        for (int t = 0; t < MT; ++t) {
          const float av = tx[(row * WLW + col) * 16 + aoff[t]];
#pragma unroll
          for (int n = 0; n < NT; ++n) acc[t][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv[n], acc[t][n], 0, 0, 0);
        }
#pragma unroll
        for (int n = 0; n < NT; ++n) acc[MT][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(1.0f, bv[n], acc[MT][n], 0, 0, 0);
      }
    }
  }
  // sum the 4 waves (K split) through LDS in wave order, then one partial per workgroup:
  // part[(blockIdx.y * gridDim.x + blockIdx.x)][10][16][CP]; D layout: rows 4*(lane>>4)+r, column lane&15
  __syncthreads();
  float *red = lds;  // 10 * 16 * CP floats <= the staging area: [tap (9 = bias)][channel of the slice][cout]
  for (int w = 0; w < 4; ++w) {
    if (wave == w) {
#pragma unroll
      for (int t = 0; t <= MT; ++t)
#pragma unroll
        for (int n = 0; n < NT; ++n)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            int slot = t * 16 + 4 * ksub + r;  // D row 4 * ksub + r of tile t
            if constexpr (PACK != 0) {
              if (t < MT) {
                const int R = 16 * t + 4 * ksub + r, tap = R / PACK;
                slot = tap < 9 ? tap * 16 + (R - tap * PACK) : -1;
              } else {
                slot = 9 * 16 + 4 * ksub + r;
              }
            }
            if (slot >= 0) {
              float *d = red + slot * CP + 16 * n + m;
              *d = (w == 0 ? 0.f : *d) + acc[t][n][r];
            }
          }
    }
    __syncthreads();
  }
  float *dst = part + (((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * (10 * 16 * CP);
  for (int e = tid; e < 10 * 16 * CP; e += 256) dst[e] = red[e];
}

// ---- the 8-output-channel layers (Cin = 4 or 8: the two full-resolution layers of the controller CNN, the last layers
// of the attention nets) on v_mfma_f32_4x4x1_16B_f32.  A 16x16x4 tile is 16 output channels wide, so with 8 of them half
// of every MFMA is padding (and 72 + 1 rows fill 6 tiles of 16): 38 % useful.  The 16-block form multiplies sixteen
// independent 4x4x1 outer products per instruction at the same flop rate (tools/mfma_4x4.hip: 123-133 TF/s): block b =
// lane / 4 takes pixel b of a run of 16, lane 4b + j supplies row 4 RB + j of the (tap, channel) rows as the A operand
// and output channel 4 CB + j as the B operand, and accumulator (RB, CB) collects the 4x4 block of dW for that pixel
// residue — (9 Cin + 1) / 4 x 2 blocks with no padding but the bias block's three empty rows.  The sixteen pixel
// residues are added up once at the end (xor-shuffles over the block index).  LDS records are 9 (Cin + 1) floats per
// pixel so that the sixteen pixels of a read fall into different banks.  Same persistent walk, partial layout and
// finishing kernels as wgrad_kernel. ----
template <int CIN>
__global__ __launch_bounds__(256, 2) void wgrad_small_kernel(const float *x, const float *du, int B, int Hs, int Ws, int H, int W,
                                                          int tiles_x, int tiles_y, int ntiles, float *part,
                                                          const float *const *xtab, const float *const *dutab, int Bseg,
                                                          int CP) {
  constexpr int SX = CIN + 1, SU = 9, NRB = (9 * CIN + 1 + 3) / 4;  // the last row block = the bias row + 3 empty rows
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float *tx = lds;                    // [WLH][WLW][SX]
  float *tu = lds + WLH * WLW * SX;   // [WTH][WTW][SU]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int blk = lane >> 2, j = lane & 3;
  f32x4 acc[NRB][2];
#pragma unroll
  for (int rb = 0; rb < NRB; ++rb) acc[rb][0] = acc[rb][1] = f32x4{0.f, 0.f, 0.f, 0.f};
  int aoff[NRB - 1];
#pragma unroll
  for (int rb = 0; rb < NRB - 1; ++rb) {
    const int R = 4 * rb + j, tap = R / CIN, ci = R - tap * CIN;
    aoff[rb] = ((tap / 3) * WLW + tap % 3) * SX + ci;
  }
  const float abias = j == 0 ? 1.0f : 0.0f;
  const int per = tiles_x * tiles_y;
  // the next tile's global loads travel in registers across the MFMA phase of the current one (as wgrad_kernel<PRE>)
  constexpr int NRX = (WLH * WLW * (CIN / 4) + 255) / 256, NRU = WTH * WTW * 2 / 256;
  f32x4 rx[NRX], ru[NRU];
  auto prefetch = [&](int tile) {
    const auto t = locate_tile(tile, per, tiles_x, x, du, xtab, dutab, Bseg);
    const int b = t.b, ty0 = t.ty0, tx0 = t.tx0;
    const float *xb = t.x, *ub = t.du;
#pragma unroll
    for (int i = 0; i < NRX; ++i) {
      const int e = tid + 256 * i;
      const int pix = e / (CIN / 4), c4 = e - pix * (CIN / 4);
      const int r = pix / WLW, c = pix - r * WLW;
      const int Y = ty0 + r - 1, X = tx0 + c - 1;
      const bool ok = (e < WLH * WLW * (CIN / 4)) & (Y >= 0) & (Y < H) & (X >= 0) & (X < W);
      const size_t off = ok ? (((size_t)b * Hs + Y) * Ws + X) * CIN + 4 * c4 : 0;
      const f32x4 v = *reinterpret_cast<const f32x4 *>(xb + off);
      rx[i] = ok ? v : f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int i = 0; i < NRU; ++i) {
      const int e = tid + 256 * i;
      const int pix = e >> 1, c4 = e & 1;
      const int r = pix / WTW, c = pix - r * WTW;
      const int Y = ty0 + r, X = tx0 + c;
      const bool ok = (Y < H) & (X < W);
      const size_t off = ok ? (((size_t)b * H + Y) * W + X) * 8 + 4 * c4 : 0;
      const f32x4 v = *reinterpret_cast<const f32x4 *>(ub + off);
      ru[i] = ok ? v : f32x4{0.f, 0.f, 0.f, 0.f};
    }
  };
  if ((int)blockIdx.x < ntiles) prefetch(blockIdx.x);
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    __syncthreads();  // the previous tile's MFMA reads are complete
#pragma unroll
    for (int i = 0; i < NRX; ++i) {
      const int e = tid + 256 * i;
      const int pix = e / (CIN / 4), c4 = e - pix * (CIN / 4);
      if (e < WLH * WLW * (CIN / 4)) {
#pragma unroll
        for (int k = 0; k < 4; ++k) tx[pix * SX + 4 * c4 + k] = rx[i][k];
      }
    }
#pragma unroll
    for (int i = 0; i < NRU; ++i) {
      const int e = tid + 256 * i;
      const int pix = e >> 1, c4 = e & 1;
#pragma unroll
      for (int k = 0; k < 4; ++k) tu[pix * SU + 4 * c4 + k] = ru[i][k];
    }
    __syncthreads();
    if (tile + (int)gridDim.x < ntiles) prefetch(tile + gridDim.x);
#pragma unroll 1
    for (int g = 0; g < 4; ++g) {  // this wave's rows 2 wave, 2 wave + 1; two runs of 16 pixels per row
      const int row = wave * 2 + (g >> 1), px = 16 * (g & 1) + blk;
      const float *ax = tx + (row * WLW + px) * SX;
      const float *bu = tu + (row * WTW + px) * SU;
      const float b0 = bu[j], b1 = bu[4 + j];
#pragma unroll
      for (int rb = 0; rb < NRB; ++rb) {
        const float a = rb < NRB - 1 ? ax[aoff[rb < NRB - 1 ? rb : 0]] : abias;
        acc[rb][0] = __builtin_amdgcn_mfma_f32_4x4x1f32(a, b0, acc[rb][0], 0, 0, 0);
        acc[rb][1] = __builtin_amdgcn_mfma_f32_4x4x1f32(a, b1, acc[rb][1], 0, 0, 0);
      }
    }
  }
  // the sixteen pixel residues (blocks) of an accumulator are added up by xor-shuffles over the block index; lanes 0..3
  // then hold D[4 rb + r][4 cb + lane] and put it into the wave's own copy of the partial record
  __syncthreads();
  // the records as wgrad_kernel writes them, in the staging area
  sum_wave_records(lds, CP, part + (size_t)blockIdx.x * record_floats(CP), [&](float *mine) {
#pragma unroll
    for (int rb = 0; rb < NRB; ++rb)
#pragma unroll
      for (int cb = 0; cb < 2; ++cb)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float v = acc[rb][cb][r];
          for (int o = 4; o < 64; o <<= 1) v += __shfl_xor(v, o, 64);
          const int slot = row_slot<CIN>(4 * rb + r);
          if (slot >= 0 && lane < 4) mine[slot * CP + 4 * cb + lane] = v;
        }
  });
}

// ---- the DMA forms' tile staging (wgrad8_kernel, wgrad8b_kernel; their comments below tell why).  Tile `tile` goes HBM -> LDS
// directly (buffer_load_dwordx4 ... lds) as 16-byte items, pixel-major as they lie in memory: XPB bytes per x pixel (tile +
// halo, dma_x_bytes), UPB per dU pixel (dma_u_bytes) at dst + dma_x_bytes.  An item outside the image reads offset kOOB, beyond
// the buffer resource's range: the hardware returns zero.  A wave's load fills 64 consecutive items; whole pieces beyond the
// x tile are skipped (wave-uniform).  Offsets are 32-bit: the host takes these forms for segments below 2 GiB.
template <int XPB, int UPB, typename P>
__device__ inline void dma_load_tile(unsigned char *dst, int tile, int per, int tiles_x, P x, P du, P const *xtab, P const *dutab,
                                     int Bseg, int bytes_x, int bytes_u, int Hs, int Ws, int H, int W) {
  constexpr int IPX = XPB / 16, IPU = UPB / 16;  // 16-byte items per pixel
  constexpr int NIX = WLH * WLW * IPX, NIU = WTH * WTW * IPU;
  constexpr int NITX = (NIX + 255) / 256, NITU = NIU / 256;
  constexpr int kOOB = 0x7fffffff;
  const int tid = threadIdx.x, wave = tid >> 6;
  const auto t = locate_tile(tile, per, tiles_x, x, du, xtab, dutab, Bseg);
  const int b = t.b, ty0 = t.ty0, tx0 = t.tx0;
  const __amdgpu_buffer_rsrc_t rsx = __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(static_cast<const void *>(t.x)), 0, bytes_x, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsu = __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(static_cast<const void *>(t.du)), 0, bytes_u, 0x00020000);
#pragma unroll
  for (int it = 0; it < NITX; ++it) {
    if (256 * it + 64 * wave >= NIX) continue;  // wave-uniform
    const int e = tid + 256 * it;
    const int pix = e / IPX, c4 = e - pix * IPX;
    const int r = pix / WLW, c = pix - r * WLW;
    const int Y = ty0 + r - 1, X = tx0 + c - 1;
    const bool ok = (e < NIX) & ((unsigned)Y < (unsigned)H) & ((unsigned)X < (unsigned)W);
    const int off = ok ? ((b * Hs + Y) * Ws + X) * XPB + 16 * c4 : kOOB;
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsx, (__attribute__((address_space(3))) void *)(dst + (256 * it + 64 * wave) * 16), 16, off, 0, 0, 0);
  }
#pragma unroll
  for (int it = 0; it < NITU; ++it) {
    const int e = tid + 256 * it;
    const int pix = e / IPU, c4 = e - pix * IPU;
    const int r = pix / WTW, c = pix - r * WTW;
    const int Y = ty0 + r, X = tx0 + c;
    const bool ok = (Y < H) & (X < W);
    const int off = ok ? ((b * H + Y) * W + X) * UPB + 16 * c4 : kOOB;
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsu, (__attribute__((address_space(3))) void *)(dst + dma_x_bytes(XPB) + (256 * it + 64 * wave) * 16), 16, off, 0, 0, 0);
  }
}

// The persistent walk of the DMA forms over two LDS buffers, ONE barrier per tile: the next tile's loads are in flight across
// the MFMAs of the current one (body(x tile, dU tile)); the barrier waits for them (vmcnt(0)) and for every wave's reads.
template <int XPB, int UPB, typename P, typename F>
__device__ inline void dma_tile_loop(unsigned char *ldsb, P x, P du, P const *xtab, P const *dutab, int B, int Bseg, int Hs, int Ws, int H,
                                     int W, int tiles_x, int tiles_y, int ntiles, F &&body) {
  constexpr int XB = dma_x_bytes(XPB), UB = dma_u_bytes(UPB);
  const int per = tiles_x * tiles_y;
  const size_t seg_imgs = xtab ? (size_t)Bseg : (size_t)B;
  const int bytes_x = (int)(seg_imgs * Hs * Ws * XPB), bytes_u = (int)(seg_imgs * H * W * UPB);
  auto load_tile = [&](int tile, int buf) {
    dma_load_tile<XPB, UPB>(ldsb + buf * (XB + UB), tile, per, tiles_x, x, du, xtab, dutab, Bseg, bytes_x, bytes_u, Hs, Ws, H, W);
  };
  int buf = 0;
  if ((int)blockIdx.x < ntiles) load_tile(blockIdx.x, 0);
  __syncthreads();
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const bool has_next = tile + (int)gridDim.x < ntiles;
    if (has_next) load_tile(tile + gridDim.x, buf ^ 1);  // in flight across the MFMAs; the barrier below waits for it
    body(ldsb + buf * (XB + UB), ldsb + buf * (XB + UB) + XB);
    __syncthreads();  // the next tile has landed (vmcnt(0)) and every wave is done reading this one
    buf ^= 1;
  }
}

// The filter gradient of the 8-output-channel full-resolution layers, third form.  wgrad_small_kernel (the 16-block MFMA)
// stages its tiles through registers with ~400 vector instructions per wave and tile, holds 38 accumulator tiles per lane
// (two waves per SIMD) and runs at 2.1-2.5 TB/s.  Measured on a first rewrite (transposed channel planes in LDS, one
// ds_read_b128 per four MFMAs): the launch is the SUM of its staging (190 us with 3/4 of the MFMAs compiled out) and its
// MFMAs (183 us) — vector instructions and MFMAs of a SIMD do not overlap (tools/mfma_valu.hip), and every workgroup of a
// CU is in the same phase.  So this form takes the vector instructions out of the staging: both tiles go HBM -> LDS
// directly (buffer_load_dwordx4 ... lds, pixel-major as they lie in memory, double-buffered, ONE barrier per tile), and
// the operands are read from there with scalar ds_reads: v_mfma_f32_16x16x4_f32 with M rows = (tap, ci) pairs + the bias
// row (A = 1), N = the 8 output channels (columns 8..15 repeat them and are dropped), k-slot (i, kq) = pixel 4 kq + i of a
// run of 16.  5 (Cin = 8) or 3 (Cin = 4) accumulator tiles.  Partial record per workgroup as wgrad_kernel writes it
// ([tap (9 = bias)][16][CP]): the same final reduction.
template <int CIN>
__global__ __launch_bounds__(256) void wgrad8_kernel(const float *x, const float *du, int B, int Hs, int Ws, int H, int W, int tiles_x,
                                                     int tiles_y, int ntiles, float *part, const float *const *xtab,
                                                     const float *const *dutab, int Bseg, int CP) {
  constexpr int NR = 9 * CIN + 1, NT = (NR + 15) / 16;  // rows: (tap, ci) pairs + bias; M tiles
  extern __shared__ __attribute__((aligned(16))) unsigned char ldsb[];  // two buffers (dma_lds_bytes), then reused for the reduction
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = lane & 15, kq = lane >> 4;
  f32x4 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  int aoff[NT];  // float offset of row R = 16 t + n inside the x tile, for pixel 4 kq of a run starting at tile column 0
  bool abias[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int R = 16 * t + n, Rc = R < 9 * CIN ? R : 0, tap = Rc / CIN, ci = Rc - tap * CIN;
    aoff[t] = ((tap / 3) * WLW + tap % 3 + 4 * kq) * CIN + ci;
    abias[t] = R == 9 * CIN;
  }
  const int boff = 4 * kq * 8 + (n & 7);
  dma_tile_loop<4 * CIN, 32>(ldsb, x, du, xtab, dutab, B, Bseg, Hs, Ws, H, W, tiles_x, tiles_y, ntiles, [&](const unsigned char *xt, const unsigned char *ut) {
    const float *xs = reinterpret_cast<const float *>(xt), *us = reinterpret_cast<const float *>(ut);
#pragma unroll
    for (int g = 0; g < 4; ++g) {  // this wave's rows 2 wave, 2 wave + 1; two runs of 16 pixels per row
      const int row = wave * 2 + (g >> 1), c0 = 16 * (g & 1);
      float bv[4], av[NT][4];
#pragma unroll
      for (int i = 0; i < 4; ++i) bv[i] = us[(row * WTW + c0 + i) * 8 + boff];
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          av[t][i] = xs[(row * WLW + c0 + i) * CIN + aoff[t]];
          if (t == NT - 1 && abias[t]) av[t][i] = 1.f;  // the bias row lives in the last tile only: one select per value there
        }
#ifdef RA_W8_SKIP  // measuring aid: one MFMA per tile and group instead of four (the LDS reads stay)
#pragma unroll
      for (int t = 0; t < NT; ++t)
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32((av[t][0] + av[t][1]) + (av[t][2] + av[t][3]), (bv[0] + bv[1]) + (bv[2] + bv[3]), acc[t], 0, 0, 0);
#else
#pragma unroll
      for (int i = 0; i < 4; ++i)  // consecutive MFMAs on different accumulators: no wait for a dependent result
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[t][i], bv[i], acc[t], 0, 0, 0);
#endif
    }
  });
  // D lane (n, q): rows 16 t + 4 q + r, column n (= output channel for n < 8)
  sum_wave_records(reinterpret_cast<float *>(ldsb), CP, part + (size_t)blockIdx.x * record_floats(CP), [&](float *mine) {
    if (n < 8) {
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int slot = row_slot<CIN>(16 * t + 4 * kq + r);
          if (slot >= 0) mine[slot * CP + n] = acc[t][r];
        }
    }
  });
}

// ... and in the bf16 mode's stacked step (round 5: x of the 8 -> 8 layer and every dU are STORED as bf16, the first layer's x is
// the float32 packed image): wgrad8b_kernel.  The bf16-operand wgrad_kernel these launches took stages float32 tiles through
// registers and ran at 242 us (8 -> 8, 43 images) / 397 us (4 -> 8, 64 images) — the 4 -> 8 one slower than the float32 mode's
// wgrad8_kernel.  Same scheme as wgrad8_kernel — both tiles HBM -> LDS directly (16 bytes per pixel each: 8 bf16 channels, or
// the 4 float32 channels of the image), double-buffered, one barrier per tile, M rows = (tap, ci) pairs + the bias row — on
// v_mfma_f32_16x16x32_bf16 with K = the 32 pixels of one tile row: a lane's operand is 8 consecutive pixels of ONE channel,
// gathered from the pixel-major tile by 8 ds_read_b32 and 4 v_perm_b32 (bf16 tiles: the low or high half of each word) or 4
// v_cvt_pk_bf16_f32 (the float32 image: rounded to nearest even, as every bf16 operand of this mode).  5 (3) MFMAs per 32
// pixels instead of 40 (24) float32 ones, half the tile bytes.  Partial records as wgrad_kernel writes them.
typedef short s16x8t __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8t __attribute__((ext_vector_type(8)));
typedef unsigned u32x4t __attribute__((ext_vector_type(4)));
template <int CIN>  // 8: x stored as bf16 (16 bytes per pixel); 4: x float32 (the packed image, 16 bytes per pixel)
__global__ __launch_bounds__(256) void wgrad8b_kernel(const void *x, const void *du, int B, int Hs, int Ws, int H, int W, int tiles_x,
                                                      int tiles_y, int ntiles, float *part, const void *const *xtab,
                                                      const void *const *dutab, int Bseg, int CP) {
  constexpr int NR = 9 * CIN + 1, NT = (NR + 15) / 16;
  extern __shared__ __attribute__((aligned(16))) unsigned char ldsb[];  // two buffers (dma_lds_bytes), then reused for the reduction
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = lane & 15, kb = lane >> 4;
  f32x4 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  // row R = 16 t + n of tile t: (tap, ci) -> byte offset of (pixel 8 kb of the row, channel ci) inside the x tile, and whether
  // the bf16 element is the high half of its word
  int aoff[NT];
  unsigned asel[NT];
  bool abias[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int R = 16 * t + n, Rc = R < 9 * CIN ? R : 0, tap = Rc / CIN, ci = Rc - tap * CIN;
    const int pix = (tap / 3) * WLW + tap % 3 + 8 * kb;
    aoff[t] = CIN == 8 ? pix * 16 + (ci >> 1) * 4 : pix * 16 + ci * 4;
    asel[t] = (ci & 1) ? 0x07060302u : 0x05040100u;  // v_perm_b32(hi word, lo word): the two high / the two low halves
    abias[t] = R == 9 * CIN;
  }
  const int co = n & 7;
  const int boff = 8 * kb * 16 + (co >> 1) * 4;
  const unsigned bsel = (co & 1) ? 0x07060302u : 0x05040100u;
  // 16 bytes per pixel in both tiles: 8 bf16 channels, or the 4 float32 channels of the image
  dma_tile_loop<16, 16>(ldsb, x, du, xtab, dutab, B, Bseg, Hs, Ws, H, W, tiles_x, tiles_y, ntiles, [&](const unsigned char *xs, const unsigned char *us) {
#pragma unroll
    for (int g = 0; g < 2; ++g) {  // this wave's rows 2 wave, 2 wave + 1: K = the row's 32 pixels
      const int row = wave * 2 + g;
      unsigned bw[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) bw[j] = *reinterpret_cast<const unsigned *>(us + (row * WTW + j) * 16 + boff);
      u32x4t bv;
#pragma unroll
      for (int j = 0; j < 4; ++j) bv[j] = __builtin_amdgcn_perm(bw[2 * j + 1], bw[2 * j], bsel);
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        u32x4t av;
        if constexpr (CIN == 8) {
          unsigned aw[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) aw[j] = *reinterpret_cast<const unsigned *>(xs + (row * WLW + j) * 16 + aoff[t]);
#pragma unroll
          for (int j = 0; j < 4; ++j) av[j] = __builtin_amdgcn_perm(aw[2 * j + 1], aw[2 * j], asel[t]);
        } else {
          float af[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) af[j] = *reinterpret_cast<const float *>(xs + (row * WLW + j) * 16 + aoff[t]);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            typedef float f32x2c __attribute__((ext_vector_type(2)));
            typedef __bf16 bf16x2c __attribute__((ext_vector_type(2)));
            av[j] = __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2c{af[2 * j], af[2 * j + 1]}, bf16x2c));
          }
        }
        if (t == NT - 1 && abias[t]) av = u32x4t{0x3f803f80u, 0x3f803f80u, 0x3f803f80u, 0x3f803f80u};  // the bias row: A = 1
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8t, av), __builtin_bit_cast(bf16x8t, bv), acc[t], 0, 0, 0);
      }
    }
  });
  sum_wave_records(reinterpret_cast<float *>(ldsb), CP, part + (size_t)blockIdx.x * record_floats(CP), [&](float *mine) {
    if (n < 8) {
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int slot = row_slot<CIN>(16 * t + 4 * kb + r);
          if (slot >= 0) mine[slot * CP + n] = acc[t][r];
        }
    }
  });
}

// dW[tap][ci][co] (= TF [3,3,Cin,Cout]) and db[co] from the partials, fixed order.
__global__ __launch_bounds__(256) void wgrad_final_kernel(const float *part, int nwg, int nchunks, int CP, int Cin, int Cout,
                                                          float *dw, float *db) {  // CP = couts per slice
  // 4 output elements per workgroup, one wave each: the 64 lanes stride over the partials, then a
  // fixed butterfly (deterministic)
  const int total = 9 * Cin * Cout + Cout;
  const int e = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (e >= total) return;
  int tap, ci, co;
  if (e < 9 * Cin * Cout) {
    co = e % Cout;
    ci = (e / Cout) % Cin;
    tap = e / (Cout * Cin);
  } else {
    tap = 9;
    ci = 0;
    co = e - 9 * Cin * Cout;
  }
  const int chunk = ci / 16, cl = ci % 16, slice = co / CP, cs = co % CP;
  float s = 0.f;
  for (int k = lane; k < nwg; k += 64)
    s += part[((((size_t)slice * nchunks + chunk) * nwg + k) * 10 + tap) * 16 * CP + cl * CP + cs];
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if (lane == 0) {
    if (tap < 9) dw[e] = s;
    else if (db) db[co] = s;
  }
}

// The same reduction, ADDED to the filter's gradient in the reference's own layout (the gradient
// bucket): [3,3,cin_w,Cout], or [3,3,Cout,cin_w] with the taps flipped for a transposed (dcnn) layer;
// chan_map sends a packed kernel channel to its filter row (-1: padding).  One writer per element.
// COALESCED reads: a lane owns one element of the record (64 consecutive floats per wave load), the four waves of a
// workgroup split the partial records and meet in LDS in a fixed order.  The wave-per-element form (wgrad_final_kernel) gives
// every lane its own record — 64 separate 4-byte loads per instruction: 96 / 107 us for the 64-channel layers' 2 048 records.
// grid (ceil(160 CP / 64), nchunks, slices).
__global__ __launch_bounds__(256) void wgrad_final_acc_rows_kernel(const float *part, int nwg, int nchunks, int CP, int Cin, int Cout,
                                                                   const int *chan_map, int cin_w, int transposed, float *gw,
                                                                   float *gb) {
  __shared__ float red[4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, rec = 160 * CP;
  const int r = blockIdx.x * 64 + lane, chunk = blockIdx.y, slice = blockIdx.z;
  float s = 0.f;
  if (r < rec) {
    const float *p = part + ((size_t)slice * nchunks + chunk) * nwg * rec + r;
    int k = wave;
    for (; k + 28 < nwg; k += 32) {  // eight loads in flight
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = p[(size_t)(k + 4 * u) * rec];
#pragma unroll
      for (int u = 0; u < 8; ++u) s += v[u];
    }
    for (; k < nwg; k += 4) s += p[(size_t)k * rec];
  }
  red[wave][lane] = s;
  __syncthreads();
  if (wave != 0 || r >= rec) return;
  s = (red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]);
  const int tap = r / (16 * CP), cl = (r / CP) & 15, cs = r % CP;
  const int ci = chunk * 16 + cl, co = slice * CP + cs;
  if (co >= Cout) return;
  if (tap == 9) {
    if (gb && chunk == 0 && cl == 0) gb[co] += s;
    return;
  }
  if (ci >= Cin) return;
  const int j = chan_map ? chan_map[ci] : (ci < cin_w ? ci : -1);
  if (j < 0) return;
  const int ky = tap / 3, kx = tap - 3 * ky;
  const size_t idx = transposed ? ((size_t)((2 - ky) * 3 + (2 - kx)) * Cout + co) * cin_w + j
                                : ((size_t)(ky * 3 + kx) * cin_w + j) * Cout + co;
  gw[idx] += s;
}

struct PtrTable {
  const float *p[64];
};
__global__ __launch_bounds__(64) void ptr_table_kernel(const PtrTable t, int n, const float **out) {
#pragma unroll
  for (int i = 0; i < 64; ++i)
    if ((int)threadIdx.x == i && i < n) out[i] = t.p[i];
}

}  // namespace train
}  // namespace ra

using namespace ra;

namespace {
// One filter-gradient request: the public entries below name what they pass, and what they leave out stays unset
struct WgradRequest {
  const char *entry = "ra_conv3x3_wgrad_f32";  // for the error text
  const void *x = nullptr, *du = nullptr;      // [B,Hs,Ws,Cin] and [B,H,W,Cout], float32 or (fmt) bf16 ...
  const void *const *xtab = nullptr, *const *dutab = nullptr;  // ... or device tables of B / Bseg segments, Bseg images each
  int Cin = 0, Cout = 0, B = 0, Bseg = 0, Hs = 0, Ws = 0, upsample = 0;
  bool bf16 = false;  // bf16 operands
  int fmt = 0;        // with them: bit 0 = x is stored as bf16, bit 1 = du
  // acc == false: dw / db are written in the kernel's own [3,3,Cin,Cout] / [Cout] layout; acc == true: the sums are added to
  // them in the reference layout (chan_map, cin_w, transposed as in wgrad_final_acc_rows_kernel)
  float *dw = nullptr, *db = nullptr;
  bool acc = false;
  const int *chan_map = nullptr;
  int cin_w = 0, transposed = 0;
  float *ws = nullptr;  // the partial records, ws_floats of them
  size_t ws_floats = 0;
  void *stream = nullptr;
  int ups() const { return upsample ? 1 : 0; }
  int H() const { return Hs * (1 + ups()); }
  int W() const { return Ws * (1 + ups()); }
  int tiles_x() const { return ceil_div(W(), train::WTW); }
  int tiles_y() const { return ceil_div(H(), train::WTH); }
  int ntiles() const { return tiles_x() * tiles_y() * B; }
};

enum class WgradFamily { generic, block16, dma_f32, dma_bf16 };  // wgrad_kernel, wgrad_small_kernel, wgrad8_kernel, wgrad8b_kernel
struct WgradForm {
  WgradFamily family;
  int NT, PACK;  // 16 NT output channels per workgroup (and per partial record); the generic kernel's packed rows
  bool BF, PRE;
  dim3 grid;     // (persistent workgroups, 16-channel chunks of Cin, 16 NT-wide slices of Cout)
  size_t lds;
  size_t ws_floats() const { return (size_t)grid.x * grid.y * grid.z * train::record_floats(16 * NT); }
};

// The launch form of a request whose shape has been checked (Cin % 4 == 0, Cout <= 128): every tuning variable and threshold
WgradForm choose_wgrad_form(const WgradRequest &r) {
  using namespace ra::train;
  // persistent workgroups: 4 per CU (38 KB of LDS each) hide the un-prefetched tile staging; 256 left 4 waves per CU
  static const int wgs_env = env_int("RA_WGRAD_WGS", 1024), wgs = wgs_env < 1 ? 1 : wgs_env;
  static const int pre_env = env_int("RA_WGRAD_PRE", 1);      // =0: tuning aid, no register prefetch of the next tile
  static const int pack_env = env_int("RA_WGRAD_PACK", 1);    // =0: tuning aid, channel rows for every Cin
  static const int small_env = env_int("RA_WGRAD_SMALL", 1);  // =0: tuning aid, the 16x16x4 form for the 8-output-channel layers too
  static const int dma_env = env_int("RA_WGRAD8", 1);  // =0: tuning aid, the 16-block form (wgrad_small_kernel) instead of the transposed-tile ones
  const int Cin = r.Cin, fmt = r.fmt, cp = ra_conv_cout_padded(r.Cout), per = cp < 64 ? cp : 64;  // per: output channels per workgroup
  const int gx = r.ntiles() < wgs ? r.ntiles() : wgs;
  // the 8-output-channel full-resolution layers have forms of their own; the DMA ones address a segment (the larger of its two
  // tensors: dU as float32) with 32-bit byte offsets and read x as it lies in memory
  const bool eight = small_env && !r.ups() && r.Cout == 8 && (Cin == 4 || Cin == 8);
  const size_t seg_bytes = (size_t)(r.xtab ? r.Bseg : r.B) * r.H() * r.W() * 8 * 4;
  const bool dma_ok = dma_env && seg_bytes < (1ull << 31) && r.Hs == r.H() && r.Ws == r.W();
  WgradForm f{WgradFamily::generic, per / 16, 0, r.bf16, false, dim3(gx), 0};
  if (eight && r.bf16 && dma_ok && (fmt & 2) && (Cin == 8) == ((fmt & 1) != 0)) {
    // bf16 mode, stacked step: dU stored as bf16 and x either stored as bf16 (8 channels) or the float32 packed image (4 channels)
    f.family = WgradFamily::dma_bf16;
    f.lds = dma_lds_bytes(16, 16, per);
  } else if (eight && !r.bf16) {
    f.family = dma_ok ? WgradFamily::dma_f32 : WgradFamily::block16;
    f.lds = dma_ok ? dma_lds_bytes(4 * Cin, 32, per) : block16_lds_bytes(Cin, per);
  } else {
    f.PACK = (pack_env && per <= 32 && (Cin == 4 || Cin == 8)) ? Cin : 0;
    f.PRE = pre_env && per <= 32 && (r.Cout & 3) == 0;
    f.grid = dim3(gx, ceil_div(Cin, 16), cp / per);
    f.lds = generic_lds_bytes(per);
  }
  return f;
}

template <int NT, int PACK, bool BF, bool PRE>
void launch_generic(const WgradForm &f, const WgradRequest &r) {
  static const MaxDynamicLds lds_limit(train::wgrad_kernel<NT, PACK, BF, PRE>, 100 * 1024);
  typedef const float *F;
  hipLaunchKernelGGL((train::wgrad_kernel<NT, PACK, BF, PRE>), f.grid, dim3(256), f.lds, as_stream(r.stream), (F)r.x, (F)r.du, r.B, r.Hs, r.Ws,
                     r.Cin, r.ups(), r.H(), r.W(), r.Cout, r.tiles_x(), r.tiles_y(), r.ntiles(), r.ws, (const F *)r.xtab, (const F *)r.dutab,
                     r.Bseg, r.fmt);
}
// A form -> its instantiation.  Contract with choose_wgrad_form: PACK and PRE are set only where NT <= 2 (it gates both on
// per <= 32); the packed and the prefetching kernels are built for those alone, and NT = 4 would drop either without a word.
template <int NT, int PACK>
void launch_generic_bf(const WgradForm &f, const WgradRequest &r) {
  if constexpr (NT <= 2) {  // the prefetching instantiations exist for these
    if (f.PRE) return f.BF ? launch_generic<NT, PACK, true, true>(f, r) : launch_generic<NT, PACK, false, true>(f, r);
  }
  f.BF ? launch_generic<NT, PACK, true, false>(f, r) : launch_generic<NT, PACK, false, false>(f, r);
}
template <int NT>
void launch_generic_pack(const WgradForm &f, const WgradRequest &r) {
  if constexpr (NT <= 2) {
    if (f.PACK) return f.PACK == 4 ? launch_generic_bf<NT, 4>(f, r) : launch_generic_bf<NT, 8>(f, r);
  }
  launch_generic_bf<NT, 0>(f, r);
}
// the 8-output-channel forms: kern = the family's instantiation for Cin = 4 or 8, P = its tensor pointer type
template <typename P, typename K>
void launch_eight(K kern, const WgradForm &f, const WgradRequest &r) {
  hipLaunchKernelGGL(kern, f.grid, dim3(256), f.lds, as_stream(r.stream), (P)r.x, (P)r.du, r.B, r.Hs, r.Ws, r.H(), r.W(), r.tiles_x(), r.tiles_y(),
                     r.ntiles(), r.ws, (const P *)r.xtab, (const P *)r.dutab, r.Bseg, 16 * f.NT);
}

void launch_wgrad_form(const WgradForm &f, const WgradRequest &r) {
  const bool c4 = r.Cin == 4;
  switch (f.family) {
    case WgradFamily::dma_bf16: launch_eight<const void *>(c4 ? train::wgrad8b_kernel<4> : train::wgrad8b_kernel<8>, f, r); break;
    case WgradFamily::dma_f32: launch_eight<const float *>(c4 ? train::wgrad8_kernel<4> : train::wgrad8_kernel<8>, f, r); break;
    case WgradFamily::block16: launch_eight<const float *>(c4 ? train::wgrad_small_kernel<4> : train::wgrad_small_kernel<8>, f, r); break;
    case WgradFamily::generic:
      if (f.NT == 1) launch_generic_pack<1>(f, r);
      else if (f.NT == 2) launch_generic_pack<2>(f, r);
      else launch_generic_pack<4>(f, r);
      break;
  }
}

int wgrad_impl(const WgradRequest &r) {
  if (r.acc && (r.cin_w <= 0 || (!r.chan_map && r.cin_w > r.Cin))) return fail(RA_E_INVALID, "%s: cin_w %d", r.entry, r.cin_w);
  if (r.fmt && !r.bf16) return fail(RA_E_INVALID, "ra_conv3x3_wgrad: bf16 storage needs the bf16-operand kernels");
  if ((r.xtab ? !r.dutab || r.Bseg <= 0 : !r.x || !r.du) || !r.ws || !r.dw || r.B <= 0 || r.Hs <= 0 || r.Ws <= 0 || r.Cin <= 0 || r.Cout <= 0)
    return fail(RA_E_INVALID, "ra_conv3x3_wgrad_f32: bad argument");
  if (r.Cin % 4 || !ra_conv_cout_padded(r.Cout)) return fail(RA_E_SHAPE, "ra_conv3x3_wgrad_f32: Cin %d %% 4 or Cout %d", r.Cin, r.Cout);
  const WgradForm f = choose_wgrad_form(r);
  if (r.ws_floats < f.ws_floats()) return fail(RA_E_WORKSPACE, "ra_conv3x3_wgrad_f32: workspace too small");
  launch_wgrad_form(f, r);
  const int per = 16 * f.NT, chunks = ceil_div(r.Cin, 16), slices = ra_conv_cout_padded(r.Cout) / per, nwg = f.grid.x;
  if (r.acc)
    hipLaunchKernelGGL(train::wgrad_final_acc_rows_kernel, dim3(ceil_div(160 * per, 64), chunks, slices), dim3(256), 0, as_stream(r.stream), r.ws,
                       nwg, chunks, per, r.Cin, r.Cout, r.chan_map, r.cin_w, r.transposed ? 1 : 0, r.dw, r.db);
  else
    hipLaunchKernelGGL(train::wgrad_final_kernel, dim3(ceil_div(9 * r.Cin * r.Cout + r.Cout, 4)), dim3(256), 0, as_stream(r.stream), r.ws, nwg,
                       chunks, per, r.Cin, r.Cout, r.dw, r.db);
  return launch_status("ra_conv3x3_wgrad_f32");
}

}  // namespace

extern "C" size_t ra_conv3x3_wgrad_workspace_floats(int Cin, int Cout, int B, int H, int W) {
  if (!ra_conv_cout_padded(Cout) || Cin <= 0 || B <= 0) return 0;
  // One record of 160 * 16 NT floats per workgroup, chunk and slice.  grid.x follows the tile count alone, and chunks * slices *
  // 16 NT = ceil(Cin / 16) * CoutP in every family (the 8-output-channel forms: one chunk, one slice of 16), so the form chosen
  // for the bare shape has the size of every launch of that shape, whatever its operand type, storage or tables.
  WgradRequest r;
  r.Cin = Cin; r.Cout = Cout; r.B = B; r.Hs = H; r.Ws = W;
  return choose_wgrad_form(r).ws_floats();
}

extern "C" int ra_conv3x3_wgrad_f32(const float *x, int Cin, int B, int Hs, int Ws, int upsample, const float *du,
                                    int Cout, float *ws, size_t ws_floats, float *dw, float *db, void *stream) {
  WgradRequest r;
  r.entry = "ra_conv3x3_wgrad_f32"; r.x = x; r.du = du; r.Cin = Cin; r.Cout = Cout; r.B = B; r.Hs = Hs; r.Ws = Ws; r.upsample = upsample;
  r.ws = ws; r.ws_floats = ws_floats; r.dw = dw; r.db = db; r.stream = stream;
  return wgrad_impl(r);
}

extern "C" int ra_conv3x3_wgrad_acc_f32(const float *x, int Cin, int B, int Hs, int Ws, int upsample, const float *du,
                                        int Cout, float *ws, size_t ws_floats, const int *chan_map, int cin_w,
                                        int transposed, float *gw, float *gb, void *stream) {
  WgradRequest r;
  r.entry = "ra_conv3x3_wgrad_acc_f32"; r.x = x; r.du = du; r.Cin = Cin; r.Cout = Cout; r.B = B; r.Hs = Hs; r.Ws = Ws; r.upsample = upsample;
  r.ws = ws; r.ws_floats = ws_floats; r.dw = gw; r.db = gb; r.stream = stream;
  r.acc = true; r.chan_map = chan_map; r.cin_w = cin_w; r.transposed = transposed;
  return wgrad_impl(r);
}

extern "C" int ra_conv3x3_wgrad_bf16ops_f32(const float *x, int Cin, int B, int Hs, int Ws, int upsample, const float *du,
                                            int Cout, float *ws, size_t ws_floats, float *dw, float *db, void *stream) {
  WgradRequest r;
  r.entry = "ra_conv3x3_wgrad_bf16ops_f32"; r.x = x; r.du = du; r.Cin = Cin; r.Cout = Cout; r.B = B; r.Hs = Hs; r.Ws = Ws; r.upsample = upsample;
  r.ws = ws; r.ws_floats = ws_floats; r.dw = dw; r.db = db; r.stream = stream; r.bf16 = true;
  return wgrad_impl(r);
}

extern "C" int ra_conv3x3_wgrad_acc_bf16ops_f32(const float *x, int Cin, int B, int Hs, int Ws, int upsample, const float *du,
                                                int Cout, float *ws, size_t ws_floats, const int *chan_map, int cin_w,
                                                int transposed, float *gw, float *gb, void *stream) {
  WgradRequest r;
  r.entry = "ra_conv3x3_wgrad_acc_bf16ops_f32"; r.x = x; r.du = du; r.Cin = Cin; r.Cout = Cout; r.B = B; r.Hs = Hs; r.Ws = Ws; r.upsample = upsample;
  r.ws = ws; r.ws_floats = ws_floats; r.dw = gw; r.db = gb; r.stream = stream; r.bf16 = true;
  r.acc = true; r.chan_map = chan_map; r.cin_w = cin_w; r.transposed = transposed;
  return wgrad_impl(r);
}

// ... and with the tensors stored as bf16 (the bf16 mode's layers between themselves): fmt bit 0 = x, bit 1 = du
extern "C" int ra_conv3x3_wgrad_acc_bf16_f32(const void *x, int Cin, int B, int Hs, int Ws, int upsample, const void *du, int Cout,
                                             float *ws, size_t ws_floats, const int *chan_map, int cin_w, int transposed, float *gw,
                                             float *gb, int fmt, void *stream) {
  WgradRequest r;
  r.entry = "ra_conv3x3_wgrad_acc_bf16_f32"; r.x = x; r.du = du; r.Cin = Cin; r.Cout = Cout; r.B = B; r.Hs = Hs; r.Ws = Ws; r.upsample = upsample;
  r.ws = ws; r.ws_floats = ws_floats; r.dw = gw; r.db = gb; r.stream = stream; r.bf16 = true; r.fmt = fmt & 3;
  r.acc = true; r.chan_map = chan_map; r.cin_w = cin_w; r.transposed = transposed;
  return wgrad_impl(r);
}

// Up to 64 device pointers (a HOST array) -> a device table, as a kernel launch (capturable in a HIP graph, where a
// host-to-device copy of pageable memory is not): the segment tables of ra_conv3x3_wgrad_multi_acc_f32.
extern "C" int ra_ptr_table(const void *const *host_ptrs, int n, void **dev_table, void *stream) {
  if (!host_ptrs || !dev_table || n <= 0 || n > 64) return fail(RA_E_INVALID, "ra_ptr_table: 1..64 pointers");
  ra::train::PtrTable t{};
  for (int i = 0; i < n; ++i) t.p[i] = static_cast<const float *>(host_ptrs[i]);
  hipLaunchKernelGGL(ra::train::ptr_table_kernel, dim3(1), dim3(64), 0, as_stream(stream), t, n,
                     (const float **)dev_table);
  return launch_status("ra_ptr_table");
}

// The filter gradient of a layer over the images of SEVERAL calls (its T timesteps in a training step) in one pass:
// xtab / dutab are device tables of nseg pointers to the calls' x [Bseg,Hs,Ws,Cin] and du [Bseg,H,W,Cout].
// bf16_operands: bit 0 = bf16 operands on the bf16 MFMA; with it, bit 1 = the x tensors are stored as bf16, bit 2 = the du tensors.
extern "C" int ra_conv3x3_wgrad_multi_acc_f32(const void *const *xtab, const void *const *dutab, int nseg, int Cin, int Bseg,
                                              int Hs, int Ws, int upsample, int Cout, float *ws, size_t ws_floats,
                                              const int *chan_map, int cin_w, int transposed, float *gw, float *gb,
                                              int bf16_operands, void *stream) {
  if (!xtab || !dutab || nseg <= 0 || Bseg <= 0) return fail(RA_E_INVALID, "ra_conv3x3_wgrad_multi_acc_f32: bad argument");
  WgradRequest r;
  r.entry = "ra_conv3x3_wgrad_multi_acc_f32"; r.xtab = xtab; r.dutab = dutab; r.Bseg = Bseg; r.B = nseg * Bseg; r.Cin = Cin; r.Cout = Cout;
  r.Hs = Hs; r.Ws = Ws; r.upsample = upsample; r.ws = ws; r.ws_floats = ws_floats; r.dw = gw; r.db = gb; r.stream = stream;
  r.bf16 = (bf16_operands & 1) != 0; r.fmt = (bf16_operands >> 1) & 3; r.acc = true; r.chan_map = chan_map; r.cin_w = cin_w; r.transposed = transposed;
  return wgrad_impl(r);
}
