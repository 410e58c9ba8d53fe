// K1 (pair form), the N-packed kernel of the first controller-CNN pair, its cache of layer A's timestep-invariant sums, and
// their entry points.  The generic pair, ra_conv_pair_f32 (which diverts here) and the plan query are in ra_conv_pair.hip;
// ra_conv_pair_parts.h holds what the two share.
#include <type_traits>

#include "ra_conv_pair_parts.h"
#include "ra_split3.h"

namespace ra {
namespace cpair {

// N-packed form for the full-resolution 8-channel pairs (controller CNN L0+L1: Cin -> 8 -> <=8,
// pool 2).  A 16x16x4 MFMA has 16 output columns; with 8 output channels half of them would
// multiply zeros.  Here the 16 columns are 2 horizontally adjacent pixels x 8 channels,
//   n = p*8 + co,  D[m][n] = sum_{ky, kx' in 0..3, ci} in[y+ky-1][x_even-1+kx'][ci] * W'[ky][kx'][ci][n],
//   W'[ky][kx'][ci][p*8+co] = W[ky][kx'-p][ci][co]  (0 outside 0 <= kx'-p <= 2),
// so one MFMA row is a pixel PAIR: 12 k-steps per 32 pixels instead of 2 x 9.  W' is built in
// registers from the standard packed filter (predicated loads), the interface does not change.
// Tile = 16 x 32 conv pixels (8 x 16 pooled).  Row mappings:
//   phase A (no pool): 21 groups of 16 (row, pixel pair) cells cover the 18 rows x 18 pairs (36 even-aligned columns) layer B
//                      reads, each cell once (NGeo::cell); result -> LDS tile `tmid`
//   phase B (pool 2):  m -> (pair m>>1, row m&1), groups of 2 rows x 16 cols; the pool window of a
//                      pair is registers (2j, 2j+1) of lanes n and n^8 -> v_max + one DPP row_ror:8.
// Both LDS tiles use odd row strides (43 / 41 pixels) so the strided operand reads are 2-way
// instead of 4-way bank-conflicted (MI355X_MICROARCH.md, LDS: bank = dword address mod 32 / 64).
template <int CINA>
struct NGeo {
  static constexpr int TH = 16, TW = 32;
  static constexpr int NCGA = CINA / 4;
  static constexpr int AW = 41, AHS = TH + 2;  // tmid: row stride (pixels), rows stored
  static constexpr int LW = 43, LH = 22;       // tin: row stride, rows addressable
  // Phase A's group map.  Layer B reads rows 0..17 x pixel pairs 0..17 of the region (pair j = region columns 2j, 2j + 1): 324
  // cells, 20.25 MFMA groups of 16.  21 groups cover them without a dead or repeated cell:
  //   0..15   interior, 4 rows x 4 pairs: group g = rows 4 (g >> 2).., pairs 4 (g & 3)..      (m -> row m >> 2, pair m & 3)
  //   16, 17  right strips, 8 rows x pairs 16, 17: rows 8 (g - 16)..                          (m -> row m >> 1, pair m & 1)
  //   18, 19  bottom strips, rows 16, 17 x 8 pairs: pairs 8 (g - 18)..                        (m -> row m >> 3, pair m & 7)
  //   20      the corner, rows 16, 17 x pairs 16, 17, in MFMA rows 0..3; rows 4..15 are spare: they repeat the cell of row
  //           m & 3 (an address inside the staged window, finite values) and are masked at every store
  // Every wave runs GPW = 5 slots: slot s < 4 is interior group 4 s + wave, slot 4 is strip 16 + wave.  Slot 5, the corner, is
  // run by ONE wave per tile, wave tile & 3 (the tile's index, so the static and the ticket walk agree).
  static constexpr int NGA = 21, GPW = 5, NSLOT = GPW + 1, AR = AHS, AP = TW / 2 + 2;  // region: AR rows x AP pairs
  struct Cell {
    int row, pair;
    bool live;
  };
  static constexpr __host__ __device__ int group_of(int wave, int s) { return s < 4 ? 4 * s + wave : s == 4 ? 16 + wave : 20; }
  // MFMA row m of slot s of wave `wave` (s == NSLOT - 1: any wave)
  static constexpr __host__ __device__ Cell cell(int wave, int s, int m) {
    if (s < 4) return Cell{4 * s + (m >> 2), 4 * wave + (m & 3), true};
    if (s == 4) return wave < 2 ? Cell{8 * wave + (m >> 1), 16 + (m & 1), true} : Cell{16 + (m >> 3), 8 * (wave - 2) + (m & 7), true};
    return Cell{16 + ((m >> 1) & 1), 16 + (m & 1), m < 4};
  }
  // the map hits each of the AR x AP cells with exactly one live MFMA row, its groups are 0 .. NGA - 1, each once, and a spare
  // row stays inside the region (so its reads stay inside the staged window)
  static constexpr bool map_exact() {
    int hits[AR * AP] = {};
    bool seen[NGA] = {};
    for (int s = 0; s < NSLOT; ++s)
      for (int w = 0; w < (s == GPW ? 1 : 4); ++w) {
        const int g = group_of(w, s);
        if (g < 0 || g >= NGA || seen[g]) return false;
        seen[g] = true;
        for (int m = 0; m < 16; ++m) {
          const Cell c = cell(w, s, m);
          if (c.row < 0 || c.row >= AR || c.pair < 0 || c.pair >= AP) return false;
          if (c.live) ++hits[c.row * AP + c.pair];
        }
      }
    for (int g = 0; g < NGA; ++g)
      if (!seen[g]) return false;
    for (int i = 0; i < AR * AP; ++i)
      if (hits[i] != 1) return false;
    return true;
  }
  static_assert(AR * AP == 324 && NGA * 16 - 12 == AR * AP, "18 rows x 18 pairs = 21 groups less the corner's 12 spare rows");
  // tin rows / cols actually loaded (20 x 38): every value that shares an MFMA row with a needed
  // output must be finite even where its weight is zero (pair 17 = columns 34|35 reads tin
  // columns 34..37; 0 * NaN would poison column 34)
  static constexpr int LHL = TH + 4, LWL = TW + 6;
  static_assert(AR - 1 + 2 < LHL && 2 * (AP - 1) + 3 < LWL && LHL <= LH && LWL <= LW, "every cell's 3 x 4 window is staged");
  static constexpr int PLANE_B = AHS * AW * 16;  // bytes of one bf16 tile [AHS][AW][8] of the SPLIT form
  // the kernel's dynamic LDS, in floats: the staged input window (CACHED: the canvas alone), then the intermediate tile(s)
  template <bool CACHED>
  static constexpr int tin_floats() {
    return (LH * LW * (CACHED ? 1 : CINA) + 3) & ~3;
  }
  template <bool SPLIT>
  static constexpr int tmid_floats() {
    return SPLIT ? 3 * PLANE_B / 4 : AHS * AW * 8;
  }
  template <bool CACHED, bool SPLIT>
  static constexpr int lds_floats() {
    return tin_floats<CACHED>() + tmid_floats<SPLIT>();
  }
};
static_assert(NGeo<4>::map_exact() && NGeo<8>::map_exact(), "phase A's groups cover the 18 x 18 pair-rows exactly once");

#ifndef RA_PAIR8_OCC
#define RA_PAIR8_OCC 3  // workgroups per CU: 3 x 38.7 KB LDS, <= 168 VGPRs (4 spills)
#endif
// tools/pair8_probe.hip builds this file with -DRA_PROBE8: every workgroup accumulates the shader-clock time its
// wave 0 spends between a few points of the tile loop and leaves the sums in ra_probe8_buf[workgroup][8]
// (-DRA_P8_NOBAR: the tile loop's barriers dropped — timing only, results wrong).
#ifdef RA_PROBE8
__device__ long long *ra_probe8_buf;
#define RA_PHASE_PROBE_BUF ra_probe8_buf
#define RA_PHASE_PROBE_WG blockIdx.x
#endif
#include "ra_phase_probe.h"
#ifdef RA_P8_NOBAR
#define RA_P8_SYNC() __builtin_amdgcn_s_waitcnt(0xc07f)  /* lgkmcnt(0) only */
#else
#define RA_P8_SYNC() __syncthreads()
#endif
// CACHED form (CINA == 4 only): of layer A's input only the canvas channel changes between
// timesteps (full_model.py:640-661,843-848), so the contribution of the image channels,
// S[pixel][co] = sum_{tap, ci != canvas} x * W (no bias, no BN), is computed ONCE per forward by
// first_cache_kernel into the accumulator layout of phase A; per timestep layer A is then
//   acc = S * scale(tt) + shift(tt)  (+)  3 MFMAs over the 3 x 4 canvas window
// instead of 12 MFMAs over the 4-channel window, and only the 4-byte canvas plane is staged.
// SPLIT form (round 5, CACHED only): layer B — 24 of the pair's 27 MFMAs per pixel group — runs on the BF16 matrix pipe at
// float32 accuracy.  A float32 value is exactly the sum of three bf16 pieces (8 + 8 + 8 mantissa bits), products of bf16
// numbers are exact in float32, and of the nine piece products of a * b six carry everything above 2^-24 of it (hh, hm, mh,
// hl, lh, mm): six v_mfma_f32_16x16x32_bf16 per K = 32 block do what eight v_mfma_f32_16x16x4_f32 do, in 41 ns of a SIMD
// instead of 108 (tools/mfma_split_probe.hip, profiles/r05_mfma_split_probe.txt: K = 576 dot products come out at 1.9e-7 of
// sum |a b| against 2.3e-7 for the float32 chain).  Phase A writes its output as three bf16 tiles [pixel][8 channels]
// (hi / mid / lo); a K = 32 block of phase B is one row ky of the 3 x 4 tap window x 8 channels, so a lane's whole A operand
// of a block and piece is ONE ds_read_b128 (lane kb = window column), and the filter is 3 x 3 x 4 registers per lane.
template <int CINA, bool CACHED, bool SPLIT = false>
__global__ __launch_bounds__(256, CACHED ? (SPLIT ? 3 : 4) : RA_PAIR8_OCC) void conv_pair8_mfma(const PArgs a, int tiles_x, int tiles_y, int ntiles) {
  using G = NGeo<CINA>;
  constexpr int NCGA = G::NCGA;
  static_assert(!CACHED || CINA == 4, "cached form: 4 input channels");
  static_assert(!SPLIT || CACHED, "the split-precision layer B exists for the cached (steady-state) form");
  constexpr int PLANE_B = G::PLANE_B;
  constexpr int RECA = CACHED ? 1 : CINA;  // floats per staged input pixel
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int IN_FLOATS = G::template tin_floats<CACHED>();
  float *tin = lds;              // [LH][LW] records [ksub][cg]  (channel = 4*cg + ksub); CACHED: the canvas only
  float *tmid = lds + IN_FLOATS;  // [AHS][AW] records [ksub][cg], 8 channels
  typedef typename vec_of<NCGA>::type avecA;

  const int tid = threadIdx.x, lane = tid & 63;
  // dynamic tile tickets (a.tickets, ra_common.h): the workgroup draws its tiles from its XCD's pool instead of walking them
  __shared__ unsigned tk_sh[2];
  TicketWalk tk;
  const bool dyn = a.tickets != nullptr;
  if (dyn) tk.issue(a.tickets, ntiles);
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int m = lane & 15, ksub = lane >> 4;  // A-operand side
  const int n = lane & 15, qo = lane >> 4;    // D side: column n = (p, co), rows 4*qo + r
  const int p = n >> 3, co = n & 7;
  const int per = tiles_x * tiles_y;

  // BN scale is folded into the weights and the shift into the accumulator's initial value, so
  // the epilogue of a value is one v_max (ReLU); FP32 MFMA shares the FP32 VALU lanes on gfx950
  // (tools/mfma_valu.hip: their times add), so every VALU instruction here costs MFMA time.
  const float scA = a.scA[co], scB = a.scB[co], shB = a.shB[co];
  const float loA = a.reluA ? 0.f : -__builtin_inff(), loB = a.reluB ? 0.f : -__builtin_inff();
  // Phase A runs its MFMAs with the operands SWAPPED (filter = A operand, pixels = B operand: the same lane contents, the other
  // argument order), so its accumulators are D^T: lane (pixel mA = lane & 15, channel block g4 = lane >> 4) holds the FOUR
  // channels 4 g4 .. 4 g4 + 3 of column n = (p, co), i.e. channels coA0 .. coA0 + 3 of ONE pixel (pixel pA of the pair-row
  // that NGeo::cell gives MFMA row mA of the group).  With pixels as rows a lane held one channel of four pixels and wrote the bf16 tiles of layer B with twelve
  // 2-byte LDS stores per group; now it is three 8-byte stores (phase A was 45 % of a workgroup's life, issue-bound on them).
  const int pA = ksub >> 1, coA0 = 4 * (ksub & 1);
  f32x4 scA4, shA4;
#pragma unroll
  for (int j = 0; j < 4; ++j) scA4[j] = a.scA[coA0 + j], shA4[j] = a.shA[coA0 + j];
  // W' of both layers, once per workgroup: one dword per (tap', cg) per lane, zero where the
  // tap misses pixel p
  // FILL (un-cached kernel with a cache pointer): the first timestep of a forward.  Its canvas is all
  // zero, so layer A's raw sums ARE the image part: they are written to the cache on the way
  // (weights left unscaled, scale / shift applied afterwards) and no separate cache kernel runs.
  const bool fill = !CACHED && a.cache != nullptr;
  float bA[CACHED ? 1 : 12][NCGA], bB[12][2];
  float bAc[3];  // CACHED: k = the 4 window columns of row ky of the canvas channel alone
#pragma unroll
  for (int ky = 0; ky < 3; ++ky) {
    const int kx = ksub - p;
    const bool ok = (kx >= 0) & (kx <= 2);
    const int tap = ok ? ky * 3 + kx : 0;
    const float w = a.wpA[((tap * NCGA + (a.plane_chan >> 2)) * 4 + (a.plane_chan & 3)) * a.CoutAP + co];
    bAc[ky] = (CACHED && ok) ? w * scA : 0.f;
  }
#pragma unroll
  for (int ky = 0; ky < 3; ++ky)
#pragma unroll
    for (int kxp = 0; kxp < 4; ++kxp) {
      const int kx = kxp - p;
      const bool ok = (kx >= 0) & (kx <= 2);
      const int tap = ok ? ky * 3 + kx : 0;
      if constexpr (!CACHED) {
#pragma unroll
        for (int cg = 0; cg < NCGA; ++cg) {
          const float w = a.wpA[((tap * NCGA + cg) * 4 + ksub) * a.CoutAP + co];
          bA[ky * 4 + kxp][cg] = ok ? w * (fill ? 1.f : scA) : 0.f;
        }
      }
#pragma unroll
      for (int cg = 0; cg < 2; ++cg) {
        const float w = a.wpB[((tap * 2 + cg) * 4 + ksub) * a.CoutBP + co];
        bB[ky * 4 + kxp][cg] = ok ? w * scB : 0.f;
      }
    }

  // SPLIT: this lane's B operands — block ky, k-slot j = input channel j of window column kb = ksub, column n = (p, co) —
  // as three bf16 pieces (the BN scale folded in before the split)
  s16x8 wB[SPLIT ? 3 : 1][SPLIT ? 3 : 1];
  if constexpr (SPLIT) {
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
      const int kx = ksub - p;
      const bool ok = (kx >= 0) & (kx <= 2);
      const int tap = ok ? ky * 3 + kx : 0;
#pragma unroll
      for (int j = 0; j < 8; j += 2) {
        const float w0 = a.wpB[((tap * 2 + (j >> 2)) * 4 + (j & 3)) * a.CoutBP + co];
        const float w1 = a.wpB[((tap * 2 + ((j + 1) >> 2)) * 4 + ((j + 1) & 3)) * a.CoutBP + co];
        unsigned H, M, L;
        split3_pair(ok ? w0 * scB : 0.f, ok ? w1 * scB : 0.f, H, M, L);
        wB[ky][0][j] = (short)(H & 0xffffu), wB[ky][0][j + 1] = (short)(H >> 16);
        wB[ky][1][j] = (short)(M & 0xffffu), wB[ky][1][j + 1] = (short)(M >> 16);
        wB[ky][2][j] = (short)(L & 0xffffu), wB[ky][2][j + 1] = (short)(L >> 16);
      }
    }
  }
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(a.src), 0, a.bytes0, 0x00020000);
  const __amdgpu_buffer_rsrc_t rp = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float *>(a.plane ? a.plane : a.src), 0, a.plane ? a.bytes_p : 0, 0x00020000);
  constexpr int NE = G::LHL * G::LWL, NIT = (NE + 255) / 256;
  // this thread's staged pixels (tile-independent): position in the loaded window and LDS record
  int e_rr[NIT], e_cc[NIT];
#pragma unroll
  for (int i = 0; i < NIT; ++i) {
    const int e = tid + 256 * i;
    e_rr[i] = e / G::LWL;
    e_cc[i] = e - e_rr[i] * G::LWL;
    if (e >= NE) e_rr[i] = -(1 << 20);  // never inside the image
  }
  // byte offset of those pixels inside the window, (rr * W + cc) * 4 (x CINA for the packed input):
  // tile-invariant, so an interior window costs ONE add per load; elements past the window carry 2^31,
  // which keeps any sum with a tile base outside the buffer (reads as 0)
  unsigned e_offp[NIT], e_offs[NIT];
#pragma unroll
  for (int i = 0; i < NIT; ++i) {
    const bool in = tid + 256 * i < NE;
    const unsigned o = (unsigned)(e_rr[i] * a.W + e_cc[i]) * 4u;
    e_offp[i] = in ? o : 0x80000000u;
    e_offs[i] = in ? o * CINA : 0x80000000u;
  }
  // tile index -> (image, tile row, tile column) without divisions in the loop: the stride gridDim.x
  // is decomposed once and added with carries (all scalar)
  struct TC {
    int b, ty, tx;
  };
  auto split = [&](int t) {
    TC c;
    c.b = t / per;
    const int r = t - c.b * per;
    c.ty = r / tiles_x;
    c.tx = r - c.ty * tiles_x;
    return c;
  };
  // tile walk: workgroup g takes tiles g, g + gridDim.x, ...; or, XCD-contiguous (a.xcd_map, gridDim.x % 8 == 0):
  // workgroups are dealt to the 8 XCDs round robin, so XCD x = g % 8 walks the tiles [x * chunk, (x + 1) * chunk) with its
  // gridDim.x / 8 workgroups — neighbouring tiles (shared halo rows, the cache's halo) then meet in ONE L2
  const int nwx = a.xcd_map ? (int)gridDim.x >> 3 : (int)gridDim.x;
  const int chunk = (ntiles + 7) >> 3;
  const int t_first = a.xcd_map ? ((int)blockIdx.x & 7) * chunk + ((int)blockIdx.x >> 3) : (int)blockIdx.x;
  const int t_end = a.xcd_map ? (((int)blockIdx.x & 7) * chunk + chunk < ntiles ? ((int)blockIdx.x & 7) * chunk + chunk : ntiles) : ntiles;
  const TC stride = split(nwx);
  auto advance = [&](TC c) {
    c.tx += stride.tx;
    if (c.tx >= tiles_x) {
      c.tx -= tiles_x;
      ++c.ty;
    }
    c.ty += stride.ty;
    if (c.ty >= tiles_y) {
      c.ty -= tiles_y;
      ++c.b;
    }
    c.b += stride.b;
    return c;
  };
  f32x4 v[NIT][NCGA];
  float pv[NIT];
  // global loads of one tile's input window (tile + halo) into registers; zeros outside the image
  auto fetch = [&](const TC &c) {
    const int fb = c.b, fy0 = c.ty * G::TH - 2, fx0 = c.tx * G::TW - 3;
    const bool inside = (fy0 >= 0) & (fy0 + G::LHL <= a.H) & (fx0 >= 0) & (fx0 + G::LWL <= a.W);
    if (inside) {  // uniform
      const unsigned base = (unsigned)((fb * a.H + fy0) * a.W + fx0) * 4u;
#pragma unroll
      for (int i = 0; i < NIT; ++i) {
        if constexpr (!CACHED) {
#pragma unroll
          for (int cg = 0; cg < NCGA; ++cg)
            v[i][cg] = __builtin_bit_cast(
                f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, (int)(base * CINA + e_offs[i] + 16u * cg), 0, 0));
        }
        pv[i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rp, (int)(base + e_offp[i]), 0, 0));
      }
      return;
    }
#pragma unroll
    for (int i = 0; i < NIT; ++i) {
      const int Y = fy0 + e_rr[i], X = fx0 + e_cc[i];
      const bool ok = (Y >= 0) & (Y < a.H) & (X >= 0) & (X < a.W);
      const int pix = (fb * a.H + Y) * a.W + X;
      if constexpr (!CACHED) {
#pragma unroll
        for (int cg = 0; cg < NCGA; ++cg)
          v[i][cg] = __builtin_bit_cast(
              f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, ok ? (pix * CINA + 4 * cg) * 4 : 0x7fffffff, 0, 0));
      }
      pv[i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rp, ok ? pix * 4 : 0x7fffffff, 0, 0));
    }
  };

  const __amdgpu_buffer_rsrc_t rc = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float *>(a.cache ? a.cache : a.src), 0, a.cache ? a.bytes_c : 0, 0x00020000);
  const int lane_b = ((m & 1) * G::AW + 2 * (m >> 1) + 1) * 8 + ksub * 2;
  const int pg = a.plane_chan >> 2, slot = a.plane_chan & 3;

  // What follows from a lane's cell (row, pixel pair of the region: NGeo::cell) in a group slot, all tile-invariant: the tin
  // record its window starts at, the byte offset of its float4 in the cache ([row][column group pair >> 2][pair & 3][n], this
  // lane's n = 4 g4 ..), and the tmid index of its pixel of the region (pixel pA of its pair).
  struct LaneCell {
    int in, c, pix;
  };
  auto lane_cell = [&](int s, int mm) {
    const typename G::Cell c = G::cell(wave, s, mm);
    return LaneCell{(c.row * G::LW + 2 * c.pair) * RECA + ksub * (CACHED ? 1 : NCGA),
                    (c.row * a.cache_gx + (c.pair >> 2)) * 256 + (c.pair & 3) * 64 + ksub * 16, c.row * G::AW + 2 * c.pair + pA};
  };
  // ... and its pixel as row | column << 8, which only a tile on the image's border asks for (it works it out per tile, as below)
  auto lane_rowcol = [&](int s) {
    int mm = m;
    asm volatile("" : "+v"(mm));
    const typename G::Cell c = G::cell(wave, s, mm);
    return c.row | (2 * c.pair + pA) << 8;
  };
  // Kept in registers for the interior slots (slot s = slot 0 moved down 4 s rows: constant and scalar offsets) and the strip
  // slot.  The corner's is worked out by the wave that runs it, per tile, from a lane index the compiler cannot see through:
  // hoisted out of the tile loop it would hold three more registers in every wave for one group in 21.
  const LaneCell cell_i = lane_cell(0, m), cell_s = lane_cell(G::GPW - 1, m);
  auto corner_cell = [&]() {
    int mm = m;
    asm volatile("" : "+v"(mm));
    return lane_cell(G::GPW, mm);
  };
  const int rows4_c = 4 * a.cache_gx * 256;  // the cache, 4 rows down
  const __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc(a.y, 0, a.bytes_y, 0x00020000);
  const unsigned lane_y = co < a.CoutB ? (unsigned)(((2 * qo + p) * a.CoutB + co) * 4) : 0x80000000u;
  int g_y[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) g_y[g] = ((g >> 1) * a.Wo + 8 * (g & 1)) * a.CoutB * 4;

  int tile = t_first;
  if (dyn) {
    tk.begin(tk_sh);
    tile = tk.cur;
  }
  bool have = dyn ? tile >= 0 : tile < t_end;
  TC cur = split(have ? tile : 0), nxt = cur;
  if (have) fetch(cur);
  RA_PHASE_DECL;
  // no group reads LDS that a tile's staging did not write (NGeo::cell: spare rows repeat a live cell); the one-time fill keeps
  // what an earlier kernel left in the rest of the window (tin rows 20, 21 and columns 38 .. 42, tmid column 40) defined
  for (int e = tid; e < G::template lds_floats<CACHED, SPLIT>() / 4; e += 256)
    reinterpret_cast<f32x4 *>(lds)[e] = f32x4{0.f, 0.f, 0.f, 0.f};
  __syncthreads();
  // the rider: this workgroup's share of the constant fill, dealt over its tiles
  const bool rider = !CACHED && a.rider_dst != nullptr;
  const __amdgpu_buffer_rsrc_t rr = __builtin_amdgcn_make_buffer_rsrc(rider ? a.rider_dst : a.y, 0,
                                                                       rider ? a.rider_quads * 16 : 0, 0x00020000);
  const int r_chunk = rider ? (a.rider_quads + (int)gridDim.x - 1) / (int)gridDim.x : 0;
  int r_idx = (int)blockIdx.x * r_chunk + tid;
  const int r_end = ((int)blockIdx.x + 1) * r_chunk < a.rider_quads ? ((int)blockIdx.x + 1) * r_chunk : a.rider_quads;
  const int my_tiles = t_end > t_first ? (t_end - t_first + nwx - 1) / nwx : 1;
  const int r_per_tile = (r_chunk + 256 * my_tiles - 1) / (256 * my_tiles);
  const u32x4 r_bits = __builtin_bit_cast(u32x4, f32x4{a.rider_val, a.rider_val, a.rider_val, a.rider_val});
  bool have_n = false;
  f32x4 cpre[CACHED ? G::NSLOT : 1];
  LaneCell cell_c{};
  auto load_cache = [&](const TC &tc, bool own) {
    const int tile_c0 = ((tc.b * a.cache_rows + tc.ty * G::TH) * a.cache_gx + ((tc.tx * G::TW) >> 3)) * 256;
#pragma unroll
    for (int s = 0; s < (CACHED ? G::GPW : 1); ++s)
      cpre[s] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(
                                              rc, tile_c0 + (s < 4 ? s * rows4_c + cell_i.c : cell_s.c), 0, 0));
    if constexpr (CACHED)
      if (own) {
        cell_c = corner_cell();
        cpre[G::GPW] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rc, tile_c0 + cell_c.c, 0, 0));
      }
  };
  for (; have; tile = dyn ? (tk.step(), tk.cur) : tile + nwx, cur = nxt, have = have_n) {
    const int b = cur.b, ty0 = cur.ty * G::TH, tx0 = cur.tx * G::TW;
    // CACHED: this tile's cached sums of layer A — 32 bytes per pixel, the launch's largest read — are requested at the top of the
    // tile, one staging pass and a barrier ahead of their use (the probe's "waiting for the cached sums 14 %"; requesting them a
    // whole phase B ahead costs more in registers than the wait: DESIGN.md, the cached first pair)
    const bool own = wave == (tile & 3);  // uniform: this wave runs the tile's 21st group, the corner
    if constexpr (CACHED) load_cache(cur, own);

    // ---------------- stage layer A's input window (prefetched registers -> LDS) ----------------
#pragma unroll
    for (int i = 0; i < NIT; ++i) {
      if constexpr (CACHED) {
        if (e_rr[i] >= 0) tin[e_rr[i] * G::LW + e_cc[i]] = pv[i];
        continue;
      }
      if (a.plane) {
#pragma unroll
        for (int cg = 0; cg < NCGA; ++cg) {  // selects, not runtime register indexing
          v[i][cg].x = (cg == pg && slot == 0) ? pv[i] : v[i][cg].x;
          v[i][cg].y = (cg == pg && slot == 1) ? pv[i] : v[i][cg].y;
          v[i][cg].z = (cg == pg && slot == 2) ? pv[i] : v[i][cg].z;
          v[i][cg].w = (cg == pg && slot == 3) ? pv[i] : v[i][cg].w;
        }
      }
      if (e_rr[i] >= 0) {
        float *rec = tin + (e_rr[i] * G::LW + e_cc[i]) * CINA;
        if constexpr (NCGA == 1) {
          *reinterpret_cast<f32x4 *>(rec) = v[i][0];
        } else {
#pragma unroll
          for (int ks = 0; ks < 4; ++ks)
#pragma unroll
            for (int cg = 0; cg < NCGA; ++cg) rec[ks * NCGA + cg] = v[i][cg][ks];
        }
      }
    }
    if (dyn) tk.publish(tk_sh);
    RA_P8_SYNC();
    RA_PHASE_AT(0);  // staged + barrier
    if (dyn) {
      tk.read_next(tk_sh);
      tk.request();  // the draw for the tile after next: older than the prefetch loads below, in flight across this tile
      have_n = tk.nxt >= 0;
      nxt = split(have_n ? tk.nxt : 0);
    } else {
      have_n = tile + nwx < t_end;
      nxt = advance(cur);
    }
    if (have_n) fetch(nxt);  // the next tile's loads fly while this one is computed
    if constexpr (!CACHED) {
      if (rider)
        for (int u = 0; u < r_per_tile; ++u, r_idx += 256)
          __builtin_amdgcn_raw_buffer_store_b128(r_bits, rr, r_idx < r_end ? r_idx * 16 : 0x7fffffff, 0, 0);
    }

    // ---------------- phase A: layer A on the 18 x 36 region -> tmid ----------------
    {
      const bool interior = (ty0 >= 1) & (ty0 + G::TH + 1 <= a.H) & (tx0 >= 2) & (tx0 + G::TW + 1 <= a.W);
      const int tile_c = ((b * a.cache_rows + ty0) * a.cache_gx + (tx0 >> 3)) * 256;  // (the FILL form's cache stores)
      // group slots S0 .. S1 - 1 of this wave: accumulators, MFMAs, epilogue and the stores to tmid (FILL: and to the cache)
      auto groups = [&](auto s0c, auto s1c, const LaneCell &edge, int rowcol_i, int rowcol_e) __attribute__((always_inline)) {
        constexpr int S0 = decltype(s0c)::value, NS = decltype(s1c)::value - S0;
        f32x4 acc[NS];
        int gin[NS];
#pragma unroll
        for (int s = 0; s < NS; ++s) gin[s] = S0 + s < 4 ? cell_i.in + 4 * (S0 + s) * G::LW * RECA : edge.in;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
          if constexpr (CACHED) {
            // this lane's 4 partial sums (columns n = 4 g4 .. + 3 of its pixel) are one float4 of the cache:
            // [image][row ty0 + row][column group tx0/8 + (pair >> 2)][pair & 3][n]
            acc[s] = cpre[S0 + s] * scA4 + shA4;
          } else {
            acc[s] = fill ? f32x4{0.f, 0.f, 0.f, 0.f} : shA4;
          }
        }
        if constexpr (S0 == 0) RA_PHASE_AT(1);  // layer A's cached sums have arrived (accumulators initialised)
        if constexpr (CACHED) {
#pragma unroll
          for (int ky = 0; ky < 3; ++ky) {
            float av[NS];
#pragma unroll
            for (int s = 0; s < NS; ++s) av[s] = tin[gin[s] + ky * G::LW];
#pragma unroll
            for (int s = 0; s < NS; ++s)
              acc[s] = __builtin_amdgcn_mfma_f32_16x16x4f32(bAc[ky], av[s], acc[s], 0, 0, 0);  // D^T: rows = (p, co), columns = pixels
          }
        } else {
#pragma unroll
          for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kxp = 0; kxp < 4; ++kxp) {
              avecA av[NS];
#pragma unroll
              for (int s = 0; s < NS; ++s)
                av[s] = *reinterpret_cast<const avecA *>(&tin[gin[s] + (ky * G::LW + kxp) * CINA]);
#pragma unroll
              for (int cg = 0; cg < NCGA; ++cg)
#pragma unroll
                for (int s = 0; s < NS; ++s)
                  acc[s] = __builtin_amdgcn_mfma_f32_16x16x4f32(bA[ky * 4 + kxp][cg], av[s][cg], acc[s], 0, 0, 0);
            }
        }
#pragma unroll
        for (int s = 0; s < NS; ++s) {
          const int S = S0 + s < 4 ? S0 + s : 0;  // (an interior slot's distance from slot 0)
          const bool inner = S0 + s < 4;
          const bool live = S0 + s < G::GPW || m < 4;  // the corner's spare rows (NGeo::cell)
          if (fill) {  // uniform: raw sums -> cache, then the folded scale / shift
            // Every live cell was computed from a complete staged window, so a tile stores all of its 18 x 18: a cell that a
            // neighbour computes too (rows 16 / 17 are the rows 0 / 1 of the tile below, pairs 16 / 17 the pairs 0 / 1 of the
            // tile on the right) gets the same bits from both, and the tiles' regions together cover the image
            const int off = live ? tile_c + (inner ? S * rows4_c + cell_i.c : edge.c) : 0x7fffffff;
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(__attribute__((ext_vector_type(4))) unsigned, acc[s]), rc, off, 0, 0);
            acc[s] = acc[s] * scA4 + shA4;
          }
          float o[4];  // channels coA0 .. coA0 + 3 of the lane's pixel
#pragma unroll
          for (int j = 0; j < 4; ++j) o[j] = fmaxf(acc[s][j], loA);
          if (!interior) {  // outside the image the intermediate is layer B's SAME padding: zero
            const int rowcol = inner ? rowcol_i + 4 * S : rowcol_e;
            const int Y = ty0 - 1 + (rowcol & 255), X = tx0 - 2 + (rowcol >> 8);
            const bool ok = (Y >= 0) & (Y < a.H) & (X >= 0) & (X < a.W);
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = ok ? o[j] : 0.f;
          }
          const int pix = inner ? cell_i.pix + 4 * S * G::AW : edge.pix;
          if constexpr (SPLIT) {
            // three bf16 tiles [pixel][channel]: the lane's four channels are 8 contiguous bytes of the pixel's record in each
            unsigned H01, M01, L01, H23, M23, L23;
            split3_pair(o[0], o[1], H01, M01, L01);
            split3_pair(o[2], o[3], H23, M23, L23);
            if (live) {
              unsigned char *d0 = reinterpret_cast<unsigned char *>(tmid) + pix * 16 + coA0 * 2;
              *reinterpret_cast<u32x2 *>(d0) = u32x2{H01, H23};
              *reinterpret_cast<u32x2 *>(d0 + PLANE_B) = u32x2{M01, M23};
              *reinterpret_cast<u32x2 *>(d0 + 2 * PLANE_B) = u32x2{L01, L23};
            }
          } else if (live) {
            // float32 tile, records [ksub][cg] (channel c at 2 (c & 3) + (c >> 2)): this lane's channels sit two floats apart
            float *dst = tmid + pix * 8 + (ksub & 1);
#pragma unroll
            for (int j = 0; j < 4; ++j) dst[2 * j] = o[j];
          }
        }
      };
      groups(std::integral_constant<int, 0>{}, std::integral_constant<int, G::GPW>{}, cell_s, interior ? 0 : lane_rowcol(0),
             interior ? 0 : lane_rowcol(G::GPW - 1));
      if (own) {
        if constexpr (!CACHED) cell_c = corner_cell();
        groups(std::integral_constant<int, G::GPW>{}, std::integral_constant<int, G::NSLOT>{}, cell_c, 0, interior ? 0 : lane_rowcol(G::GPW));
      }
    }
    RA_PHASE_AT(2);  // phase A computed and written to the LDS tile
    RA_P8_SYNC();
    RA_PHASE_AT(3);  // barrier

    // ---------------- phase B: layer B out of tmid, BN + ReLU + 2x2 max-pool -> global ----------------
    {
      f32x4 acc[4];
      int gmid[4];
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int gy = 2 * wave + (g >> 1), gx = g & 1;
        gmid[g] = (2 * gy * G::AW + 16 * gx) * 8 + lane_b;
        acc[g] = f32x4{shB, shB, shB, shB};
      }
      if constexpr (SPLIT) {
        // lane (m, kb): pixel (row (m & 1) + ky, column 2 (m >> 1) + 1 + kb) of the group, its 8 channels = one 16-byte read
        const unsigned char *tb = reinterpret_cast<const unsigned char *>(tmid);
        const int lane_px = ((m & 1) * G::AW + 2 * (m >> 1) + 1 + ksub) * 16;
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
          for (int gh = 0; gh < 2; ++gh) {  // two pixel groups at a time: 24 operand registers in flight instead of 48
            s16x8 av[2][3];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
              const int g = 2 * gh + u;
              const int gy = 2 * wave + (g >> 1), gx = g & 1;
              const int off = ((2 * gy + ky) * G::AW + 16 * gx) * 16 + lane_px;
#pragma unroll
              for (int pc = 0; pc < 3; ++pc) av[u][pc] = *reinterpret_cast<const s16x8 *>(tb + off + pc * PLANE_B);
            }
            // six piece products per block, smallest first; consecutive MFMAs alternate between the two accumulators
            constexpr int PA[6] = {1, 0, 2, 0, 1, 0}, PB[6] = {1, 2, 0, 1, 0, 0};
#pragma unroll
            for (int t = 0; t < 6; ++t)
#pragma unroll
              for (int u = 0; u < 2; ++u)
                acc[2 * gh + u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, av[u][PA[t]]),
                                                                          __builtin_bit_cast(bf16x8, wB[ky][PB[t]]), acc[2 * gh + u], 0, 0, 0);
          }
      } else {
#pragma unroll
      for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kxp = 0; kxp < 4; ++kxp) {
          f32x2 av[4];
#pragma unroll
          for (int g = 0; g < 4; ++g)
            av[g] = *reinterpret_cast<const f32x2 *>(&tmid[gmid[g] + (ky * G::AW + kxp) * 8]);
#pragma unroll
          for (int cg = 0; cg < 2; ++cg)
#pragma unroll
            for (int g = 0; g < 4; ++g)
              acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[g][cg], bB[ky * 4 + kxp][cg], acc[g], 0, 0, 0);
        }
      }
      const int prow0 = (ty0 >> 1) + wave * 2, pcol0 = (tx0 >> 1) + 2 * qo + p;
      const bool whole = ((ty0 >> 1) + G::TH / 2 <= a.Ho) & ((tx0 >> 1) + G::TW / 2 <= a.Wo);  // uniform
      const unsigned tile_y = (unsigned)(((b * a.Ho + prow0) * a.Wo + (tx0 >> 1)) * a.CoutB * 4) + lane_y;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        // ReLU commutes with max: pool first.  registers (2j, 2j+1) = rows (0, 1) of pair
        // 2*qo + j; lane n^8 holds the pair's other pixel
        const float t0 = fmaxf(fmaxf(acc[g][0], acc[g][1]), loB), t1 = fmaxf(fmaxf(acc[g][2], acc[g][3]), loB);
        const float u0 = fmaxf(t0, __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, t0), 0x128, 0xf, 0xf, true)));
        const float u1 = fmaxf(t1, __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, t1), 0x128, 0xf, 0xf, true)));
        const float ov = p ? u1 : u0;  // lane (p, co) stores pooled pixel 2*qo + p
        const int prow = prow0 + (g >> 1), pcol = pcol0 + 8 * (g & 1);
        unsigned off = tile_y + (unsigned)g_y[g];
        if (!whole) off = ((prow < a.Ho) & (pcol < a.Wo)) ? off : 0x80000000u;
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, ov), ry, (int)off, 0, 0);
      }
    }
    RA_PHASE_AT(4);  // phase B, pooled and stored
  }
  RA_PHASE_END;
  if constexpr (!CACHED) {
    if (rider)  // what rounding left of this workgroup's share (and all of it for a workgroup without tiles)
      for (; r_idx < r_end; r_idx += 256) __builtin_amdgcn_raw_buffer_store_b128(r_bits, rr, r_idx * 16, 0, 0);
  }
}

template <int CINA, bool CACHED = false, bool SPLIT = false>
int launch8(PArgs a, int B, hipStream_t st, int *plan) {
  using G = NGeo<CINA>;
  a.bytes_y = (int)((size_t)B * a.Ho * a.Wo * a.CoutB * sizeof(float));
  auto kern = conv_pair8_mfma<CINA, CACHED, SPLIT>;
  constexpr size_t lds = (size_t)G::template lds_floats<CACHED, SPLIT>() * sizeof(float);
  const int tiles_x = ceil_div(a.W, G::TW), tiles_y = ceil_div(a.H, G::TH);
  const int ntiles = tiles_x * tiles_y * B;
  // RA_PAIR8_WGS: tuning aid, persistent workgroups (default 3 per CU).  The cached form (122 VGPRs) could run 4 workgroups
  // per CU and is 0.3 us faster alone that way, but 3 leave room for the kernels of the other decode graphs: 50.4k vs 49.7k
  // instance-timesteps/s with four batches in flight
  static const int wgs = env_int("RA_PAIR8_WGS", 768);
  static const int xcd = env_int("RA_PAIR8_XCD", 1);  // =0: tuning aid, the interleaved tile walk (51.7k vs 52.1k instance-timesteps/s pipelined)
  const int grid = ntiles < wgs ? ntiles : wgs;
  a.xcd_map = (xcd && grid % 8 == 0 && grid >= 8) ? 1 : 0;
  const bool draws = CACHED && ntiles >= kTicketMinTilesPerWg * grid;  // the steady-state form; bound scratch only
  if (plan) {  // ra_conv_pair_plan: no device fact in this form's choices
    plan[RA_PLAN_FAMILY] = RA_PLAN_FAMILY_PAIR;
    plan[RA_PLAN_FORM] = RA_PLAN_FORM_NPACKED | (CACHED ? RA_PLAN_FORM_CACHED : 0) | (SPLIT ? RA_PLAN_FORM_SPLIT : 0);
    plan[RA_PLAN_CK] = CINA, plan[RA_PLAN_CMID] = 8, plan[RA_PLAN_KF] = 3, plan[RA_PLAN_TILE_H] = G::TH, plan[RA_PLAN_TILE_W] = G::TW;
    plan[RA_PLAN_TILES_X] = tiles_x, plan[RA_PLAN_TILES_Y] = tiles_y, plan[RA_PLAN_TICKETS] = draws ? 1 : 0;
    plan_walk(plan, ntiles, grid, a.xcd_map);
    return 0;
  }
  static const MaxDynamicLds lds_limit(kern, lds);
  a.tickets = draws ? take_ticket_slots(1, grid) : nullptr;
  hipLaunchKernelGGL(kern, dim3(grid), dim3(256), lds, st, a, tiles_x, tiles_y, ntiles);
  return launch_status("ra_conv_pair_f32");
}

// Timestep-invariant partial sums of the N-packed pair's layer A (see conv_pair8_mfma, CACHED):
//   S[b][Y+1][gx][r][n = p*8 + co] = sum_{ky,kx} sum_{ci != plane_chan} x[b][Y+ky-1][X+kx-1][ci] * W[ky][kx][ci][co]
// with X = 8*gx - 2 + 2*r + p (SAME zero padding; 0 for pixels outside the image), i.e. exactly
// the float4 a lane of phase A initialises its accumulator with.  The cache must be zero-filled when
// allocated: entries outside the image are never written.
__global__ __launch_bounds__(256) void first_cache_kernel(const float *x, const float *wpA, int CoutAP, int plane_chan,
                                                          int B, int H, int W, int rows, int ngx, float *cache) {
  // a workgroup = 4 image rows x 64 columns starting at X = 64*bx - 2, i.e. 8 complete column
  // groups of the cache.  One thread per pixel computes all 8 output channels (9 float4 loads,
  // 27 x 8 FMAs with wave-uniform weights), the block is transposed through LDS and written as
  // coalesced float4 [n][r] records.
  __shared__ float sm[4][64][9];  // +1: conflict-free transposed reads
  const int xl = threadIdx.x & 63, yl = threadIdx.x >> 6;
  const int X = blockIdx.x * 64 - 2 + xl, Y = blockIdx.y * 4 + yl, b = blockIdx.z;
  float acc[8];
#pragma unroll
  for (int co = 0; co < 8; ++co) acc[co] = 0.f;
  if (X >= 0 && X < W && Y < H) {
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
      const int yy = Y + ky - 1;
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const int xx = X + kx - 1;
        const bool ok = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W);
        f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
        if (ok) v = *reinterpret_cast<const f32x4 *>(x + ((size_t)(b * H + yy) * W + xx) * 4);
        const float *wt = wpA + (size_t)((ky * 3 + kx) * 4) * CoutAP;
#pragma unroll
        for (int ci = 0; ci < 4; ++ci) {
          const float xv = ci == plane_chan ? 0.f : v[ci];
#pragma unroll
          for (int co = 0; co < 8; ++co) acc[co] = fmaf(xv, wt[ci * CoutAP + co], acc[co]);
        }
      }
    }
  }
#pragma unroll
  for (int co = 0; co < 8; ++co) sm[yl][xl][co] = acc[co];
  __syncthreads();
  for (int e = threadIdx.x; e < 4 * 8 * 16; e += 256) {
    const int n4 = e & 3, r = (e >> 2) & 3, g = (e >> 4) & 7, row = e >> 7;  // columns n = 4 n4 .. 4 n4 + 3 of pair r
    const int p = n4 >> 1, co0 = 4 * (n4 & 1);
    const int Yo = blockIdx.y * 4 + row, gx = blockIdx.x * 8 + g;
    if (Yo < H && gx < ngx) {
      f32x4 o;
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = sm[row][8 * g + 2 * r + p][co0 + j];
      *reinterpret_cast<f32x4 *>(cache + (((size_t)b * rows + (Yo + 1)) * ngx + gx) * 64 + r * 16 + 4 * n4) = o;
    }
  }
}

void cache_dims(int H, int W, int &rows, int &ngx) {
  rows = ceil_div(H, NGeo<4>::TH) * NGeo<4>::TH + 4;
  ngx = ceil_div(W, NGeo<4>::TW) * (NGeo<4>::TW / 8) + 1;
}
int launch_npacked(const PArgs &a, int B, hipStream_t st, int *plan) {
  return a.C0 == 4 ? launch8<4>(a, B, st, plan) : launch8<8>(a, B, st, plan);
}

// The first timestep of a forward: the plain kernel on a zero canvas, which leaves layer A's image part in the cache on the way;
// optionally with a constant fill of another buffer riding on the launch.
int fill_cache_entry(const float *src, const float *plane, int plane_chan, int B, int H, int W, const float *wpA, const float *scaleA,
                     const float *shiftA, int reluA, const float *wpB, const float *scaleB, const float *shiftB, int CoutB, int reluB,
                     float *cache, float *y, float *fill_dst, size_t fill_floats, float fill_value, void *stream, int *plan) {
  if (missing_pointer(plan, {src, plane, cache, wpA, scaleA, shiftA, wpB, scaleB, shiftB, y}) || B <= 0)
    return fail(RA_E_INVALID, "ra_conv_pair_fill_cache_f32: bad argument");
  if (fill_dst && ((reinterpret_cast<uintptr_t>(fill_dst) & 15) || (fill_floats & 3) || fill_floats * 4 >= (1ull << 31)))
    return fail(RA_E_SHAPE, "ra_conv_pair_fill_cache_rider_f32: the fill must be 16-byte aligned, a multiple of 4 floats, < 2 GiB");
  if (!ra_conv_first_cache_supported(4, 8, CoutB, 2, H, W) || plane_chan < 0 || plane_chan > 3)
    return fail(RA_E_SHAPE, "ra_conv_pair_fill_cache_f32: unsupported shape");
  PArgs a = pair_args(src, 4, B, H, W, 0, wpA, scaleA, shiftA, 8, reluA, wpB, scaleB, shiftB, CoutB, reluB, 2, plane, plane_chan, y);
  const size_t b0 = (size_t)B * H * W * 4 * sizeof(float);
  if (b0 >= (1ull << 31)) return fail(RA_E_SHAPE, "ra_conv_pair_fill_cache_f32: input exceeds 2 GiB");
  a.bytes0 = (int)b0;
  if (int rc = pair_args_cache(a, cache, B, "ra_conv_pair_fill_cache_f32")) return rc;
  a.rider_dst = fill_floats ? fill_dst : nullptr;
  a.rider_quads = (int)(fill_floats / 4);
  a.rider_val = fill_value;
  return launch8<4, false>(a, B, as_stream(stream), plan);
}

// Every later timestep: layer A from the cached sums and the canvas plane.
int cached_entry(const float *cache, const float *plane, int plane_chan, int B, int H, int W, const float *wpA, const float *scaleA,
                 const float *shiftA, int reluA, const float *wpB, const float *scaleB, const float *shiftB, int CoutB, int reluB,
                 float *y, void *stream, int *plan) {
  if (missing_pointer(plan, {cache, plane, wpA, scaleA, shiftA, wpB, scaleB, shiftB, y}) || B <= 0)
    return fail(RA_E_INVALID, "ra_conv_pair_cached_f32: bad argument");
  if (!ra_conv_first_cache_supported(4, 8, CoutB, 2, H, W) || plane_chan < 0 || plane_chan > 3)
    return fail(RA_E_SHAPE, "ra_conv_pair_cached_f32: unsupported shape");
  // src: unused by the cached form (only the canvas plane is staged), and bytes0 stays 0
  PArgs a = pair_args(plane, 4, B, H, W, 0, wpA, scaleA, shiftA, 8, reluA, wpB, scaleB, shiftB, CoutB, reluB, 2, plane, plane_chan, y);
  if (int rc = pair_args_cache(a, cache, B, "ra_conv_pair_cached_f32")) return rc;
  static const int split = env_int("RA_PAIR8_SPLIT", 1);  // =0: layer B on the float32 MFMA (rounds 2-4) instead of the split-precision bf16 form
  if (split) return launch8<4, true, true>(a, B, as_stream(stream), plan);
  return launch8<4, true>(a, B, as_stream(stream), plan);
}

}  // namespace cpair
}  // namespace ra

using namespace ra;

// ---------------------------------------------------------------------------------------------
// CACHED form of the N-packed first pair (controller CNN L0 + L1 on the 4-channel packed image):
// ra_conv_first_cache_f32 once per forward, ra_conv_pair_cached_f32 per timestep.
extern "C" int ra_conv_first_cache_supported(int Cin, int CoutA, int CoutB, int poolB, int H, int W) {
  return Cin == 4 && CoutA == 8 && CoutB >= 1 && CoutB <= 8 && poolB == 2 && W > 16 && !((H | W) & 1);
}

extern "C" size_t ra_conv_first_cache_floats(int B, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0) return 0;
  int rows, ngx;
  cpair::cache_dims(H, W, rows, ngx);
  return (size_t)B * rows * ngx * 64;
}

extern "C" int ra_conv_first_cache_f32(const float *src, int B, int H, int W, const float *wpA, int CoutA,
                                       int plane_chan, float *cache, void *stream) {
  if (!src || !wpA || !cache || B <= 0 || H <= 0 || W <= 0 || plane_chan < 0 || plane_chan > 3)
    return fail(RA_E_INVALID, "ra_conv_first_cache_f32: bad argument");
  if (CoutA != 8) return fail(RA_E_SHAPE, "ra_conv_first_cache_f32: CoutA %d", CoutA);
  int rows, ngx;
  cpair::cache_dims(H, W, rows, ngx);
  const size_t total = (size_t)B * rows * ngx * 16;
  if (total * 16 >= (1ull << 31)) return fail(RA_E_SHAPE, "ra_conv_first_cache_f32: cache exceeds 2 GiB");
  hipLaunchKernelGGL(cpair::first_cache_kernel, dim3(ceil_div(W + 2, 64), ceil_div(H, 4), B), dim3(256), 0,
                     as_stream(stream), src, wpA, ra_conv_cout_padded(CoutA), plane_chan, B, H, W, rows, ngx, cache);
  return launch_status("ra_conv_first_cache_f32");
}

extern "C" int ra_conv_pair_fill_cache_rider_f32(const float *src, const float *plane, int plane_chan, int B, int H, int W,
                                                 const float *wpA, const float *scaleA, const float *shiftA, int reluA,
                                                 const float *wpB, const float *scaleB, const float *shiftB, int CoutB,
                                                 int reluB, float *cache, float *y, float *fill_dst, size_t fill_floats,
                                                 float fill_value, void *stream) {
  return cpair::fill_cache_entry(src, plane, plane_chan, B, H, W, wpA, scaleA, shiftA, reluA, wpB, scaleB, shiftB, CoutB, reluB, cache, y,
                                 fill_dst, fill_floats, fill_value, stream, nullptr);
}

extern "C" int ra_conv_pair_fill_cache_f32(const float *src, const float *plane, int plane_chan, int B, int H, int W,
                                           const float *wpA, const float *scaleA, const float *shiftA, int reluA,
                                           const float *wpB, const float *scaleB, const float *shiftB, int CoutB,
                                           int reluB, float *cache, float *y, void *stream) {
  return ra_conv_pair_fill_cache_rider_f32(src, plane, plane_chan, B, H, W, wpA, scaleA, shiftA, reluA, wpB, scaleB, shiftB,
                                           CoutB, reluB, cache, y, nullptr, 0, 0.0f, stream);
}

extern "C" int ra_conv_pair_cached_f32(const float *cache, const float *plane, int plane_chan, int B, int H, int W,
                                       const float *wpA, const float *scaleA, const float *shiftA, int reluA,
                                       const float *wpB, const float *scaleB, const float *shiftB, int CoutB,
                                       int reluB, float *y, void *stream) {
  return cpair::cached_entry(cache, plane, plane_chan, B, H, W, wpA, scaleA, shiftA, reluA, wpB, scaleB, shiftB, CoutB, reluB, y, stream,
                             nullptr);
}
