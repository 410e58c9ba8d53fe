// K1p16 — the fused layer pair 8 -> 16 -> 16 (3x3 SAME, BN + ReLU after each layer, 2x2 max-pool after layer B: the controller
// CNN's L2+L3 at the CVPPP arch) with BOTH layers direct on the bf16 matrix pipe at float32 accuracy.
//
// Why: K1pw (conv_pair_wino_mfma<8, true>, ra_conv_wino.hip) keeps layer B as Winograd F(2x2, 3x3) on the float32 MFMA.  Since
// layer A moved to the bf16 pipe (three exact bf16 pieces per operand, six piece products per K = 32 block) a direct layer B
// costs the same matrix time — 2 groups x 5 blocks x 6 products x 16 cycles = 960 cycles per wave and 8 x 16 tile against
// 32 float32 MFMAs x 32 cycles = 1024 — and none of Winograd's overhead: no input / output transform on the VALU, no exchange
// buffer with its four barriers per tile, no LDS round trip of the accumulators, and layer A's output is read as ds_read_b128.
//
// Structure (that of conv_pair_wino_mfma<8, true>): a persistent grid, the XCD-contiguous tile walk, optional tile tickets, the
// next tile's input prefetched into registers behind both compute phases, the 12 x 20 input window staged once as three bf16
// tiles of 16-byte records, layer A over the 10 x 18 window in 12 groups of 16 pixels with swapped operands.
//   * Layer A's epilogue writes the BN + ReLU'd window, zero outside the image (layer B's SAME padding), straight as three bf16
//     tiles [window pixel][16 channels] (32-byte records).
//   * Layer B: the tile's 128 conv pixels are 8 groups of 16, two per wave (wave p = pool row p, its left and right half).  MFMA
//     row m of a group is position m & 3 of pool window m >> 2, so a lane's four accumulator registers are the four pixels of
//     ONE pool window: the pool is three v_max in registers and a pooled pixel's 16 channels leave as one 64-byte row.  A
//     K = 32 block is two taps x 16 channels: lane (m, ksub) reads channel half ksub & 1 of tap 2 blk + (ksub >> 1) of its pixel,
//     one ds_read_b128 per piece; the fifth block's second tap carries zero weights (and reads tap 8 again: finite data).
//     The folded BN scale (either sign) is in the filter pieces and the shift in the accumulator's initial value, so
//     max-then-ReLU is all that follows the MFMAs.
//   * LDS image of the window: rows are 24 records (768 bytes) apart and the two 16-byte halves of a record are swapped in odd
//     window rows.  ds_read_b128 is served in groups of 16 lanes that hold, for each of a group's four pool windows, one
//     channel half of its 2 x 2 pixels: with rows a multiple of 256 bytes apart, the window's two row-0 pixels take two of its
//     four 16-byte bank slots and the swapped halves of row 1 the other two — every group reads 16 distinct slots.
// LDS: 3 x 3840 bytes of input pieces + 3 x 7680 of window pieces + 15360 of layer B's filter pieces = 49920 bytes, three
// workgroups per CU.  Layer A's filter pieces (36 VGPRs per lane) stay in registers for the whole launch; layer B's 60 beside
// them leave the kernel with scratch at the 168 VGPRs of three workgroups per CU (profiles/pair16_direct.txt), so a wave reads
// them per block as B operands (15 ds_read_b128 per tile, shared by its two groups).
// tools/pair16_probe.hip builds this file with -DRA_PROBE16: wave 0 of every workgroup accumulates the shader-clock time between
// the points of the tile loop and leaves the sums in ra_probe16_buf[workgroup][8] (ra_phase_probe.h).
#include "ra_common.h"
#include "ra_split3.h"

#ifndef RA_PAIR16_OCC
#define RA_PAIR16_OCC 3  // workgroups per CU the register budget is cut for
#endif
namespace ra {
namespace cpair {

constexpr int P16_TSY = 8, P16_TS = 16;          // output tile (conv pixels)
constexpr int P16_WS = P16_TS + 2;               // layer-A output window width
constexpr int P16_AWY = P16_TSY + 2;             // ... and height
constexpr int P16_IWY = P16_TSY + 4, P16_IWX = P16_TS + 4;  // input window
constexpr int P16_WST = 24;                      // records between window rows in LDS
constexpr int P16_PLI = P16_IWY * P16_IWX * 16;  // bytes of one bf16 input tile [pixel][8]
constexpr int P16_PLW = P16_AWY * P16_WST * 32;  // bytes of one bf16 window tile [row][24][16]
constexpr int P16_WB = 5 * 3 * 64 * 16;          // bytes of layer B's filter pieces [block][piece][lane]
constexpr size_t P16_LDS = 3 * (size_t)(P16_PLI + P16_PLW) + P16_WB;

struct P16Args {
  const float *x, *wpA, *scA, *shA, *wpB, *scB, *shB;
  float *y;
  int B, H, W, CoutAP, CoutBP, reluA, reluB;
  int bytes_x;
  int xcd_map;
  unsigned *tickets;  // this launch's slot of tile-ticket pools (ra_common.h); nullptr = the static walk
};

// XCD-contiguous tile walk (as conv_pair_wino_mfma's): first / end / step of this workgroup's walk
struct P16Walk {
  int first, end, step;
};
__device__ inline P16Walk p16_tile_walk(int ntiles, int xcd_map) {
  P16Walk w;
  if (!xcd_map) {
    w.first = blockIdx.x;
    w.end = ntiles;
    w.step = gridDim.x;
    return w;
  }
  const int chunk = (ntiles + 7) >> 3, x = blockIdx.x & 7;
  w.first = x * chunk + ((int)blockIdx.x >> 3);
  w.end = (x * chunk + chunk < ntiles) ? x * chunk + chunk : ntiles;
  w.step = (int)gridDim.x >> 3;
  return w;
}

#ifdef RA_PROBE16
__device__ long long *ra_probe16_buf;
#define RA_PHASE_PROBE_BUF ra_probe16_buf
#define RA_PHASE_PROBE_WG blockIdx.x
#endif
#include "ra_phase_probe.h"

__global__ __launch_bounds__(256, RA_PAIR16_OCC) void conv_pair16_mfma(const P16Args a, int tiles_x, int tiles_y, int ntiles) {
  constexpr int TSY = P16_TSY, TS = P16_TS, WS = P16_WS, AWY = P16_AWY, IWX = P16_IWX, WST = P16_WST, CINA = 8;
  constexpr int NPA = AWY * WS, NGA = (NPA + 15) / 16, GPW = (NGA + 3) / 4;  // 180 window pixels, 12 groups, 3 per wave
  constexpr int NPI = P16_IWY * IWX, NIT = (NPI * 2 + 255) / 256;            // input items: (pixel, half of its 8 channels)
  constexpr int PLI = P16_PLI, PLW = P16_PLW;
  static_assert(NGA == 4 * GPW, "layer A's groups divide among the four waves");
  // dynamic tile tickets (a.tickets): tiles are drawn from this XCD's pool instead of walked (static: tile += tw.step)
  __shared__ unsigned tk_sh[2];
  TicketWalk tk;
  const bool dyn = a.tickets != nullptr;
  if (dyn) tk.issue(a.tickets, ntiles);
  extern __shared__ __attribute__((aligned(16))) unsigned char lds16[];
  unsigned char *tinp = lds16;            // three tiles [IWY][IWX] of 16-byte records: the input's 8 channels as bf16 pieces
  unsigned char *twin = lds16 + 3 * PLI;  // three tiles [AWY][WST] of 32-byte records: layer A's output, halves swapped in odd rows
  unsigned char *twb = twin + 3 * PLW;    // layer B's filter pieces
  const int tid = threadIdx.x, lane = tid & 63;
  const int p = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int m = lane & 15, ksub = lane >> 4;
  const int per = tiles_x * tiles_y;

  // layer A's filter: block blk, k-slot j = input channel j of tap 4 blk + ksub, row m (an output channel), three pieces; the BN
  // scale is folded in before the split and the shift is the accumulator's initial value, so the epilogue starts at the ReLU
  s16x8 wA[3][3];
  const float scA = a.scA[m];
#pragma unroll
  for (int blk = 0; blk < 3; ++blk) {
    const int tap = 4 * blk + ksub;
    const bool ok = tap < 9;
    const int tp = ok ? tap : 0;
#pragma unroll
    for (int j = 0; j < 8; j += 2) {
      const float w0 = a.wpA[(size_t)((tp * 2 + (j >> 2)) * 4 + (j & 3)) * a.CoutAP + m];
      const float w1 = a.wpA[(size_t)((tp * 2 + ((j + 1) >> 2)) * 4 + ((j + 1) & 3)) * a.CoutAP + m];
      unsigned H, M, L;
      split3_pair(ok ? w0 * scA : 0.f, ok ? w1 * scA : 0.f, H, M, L);
      wA[blk][0][j] = (short)(H & 0xffffu), wA[blk][0][j + 1] = (short)(H >> 16);
      wA[blk][1][j] = (short)(M & 0xffffu), wA[blk][1][j + 1] = (short)(M >> 16);
      wA[blk][2][j] = (short)(L & 0xffffu), wA[blk][2][j + 1] = (short)(L >> 16);
    }
  }
  // Layer A's MFMAs run with the operands swapped (filter = A operand, window pixels = B operand), so a lane's accumulator
  // holds channels 4 ksub .. 4 ksub + 3 of ONE window pixel (16 g + m): 8 contiguous bytes of its record in each piece
  f32x4 shA4;
#pragma unroll
  for (int j = 0; j < 4; ++j) shA4[j] = a.shA[4 * ksub + j];
  const float loA = a.reluA ? 0.f : -__builtin_inff();
  // layer B's filter: block blk, k-slot j = channel 8 (ksub & 1) + j of tap 2 blk + (ksub >> 1), column m (an output channel),
  // the BN scale folded in before the split (its sign is free: the max-pool follows the scale).  Its 60 registers per lane do
  // not fit beside layer A's at three workgroups per CU, so the pieces live in LDS as B operands [block][piece][lane], split
  // once per workgroup (wave blk & 3 makes block blk; the staging barrier of the first tile publishes them)
  {
    const float scB = a.scB[m];
#pragma unroll
    for (int blk = 0; blk < 5; ++blk) {
      if ((blk & 3) != p) continue;  // wave-uniform
      const int tap = 2 * blk + (ksub >> 1);
      const bool ok = tap < 9;
      const int tp = ok ? tap : 0;
      s16x8 w[3];
#pragma unroll
      for (int j = 0; j < 8; j += 2) {
        const int c = 8 * (ksub & 1) + j;
        const float w0 = a.wpB[(size_t)((tp * 4 + (c >> 2)) * 4 + (c & 3)) * a.CoutBP + m];
        const float w1 = a.wpB[(size_t)((tp * 4 + ((c + 1) >> 2)) * 4 + ((c + 1) & 3)) * a.CoutBP + m];
        unsigned H, M, L;
        split3_pair(ok ? w0 * scB : 0.f, ok ? w1 * scB : 0.f, H, M, L);
        w[0][j] = (short)(H & 0xffffu), w[0][j + 1] = (short)(H >> 16);
        w[1][j] = (short)(M & 0xffffu), w[1][j + 1] = (short)(M >> 16);
        w[2][j] = (short)(L & 0xffffu), w[2][j + 1] = (short)(L >> 16);
      }
#pragma unroll
      for (int pc = 0; pc < 3; ++pc) *reinterpret_cast<s16x8 *>(twb + ((blk * 3 + pc) * 64 + lane) * 16) = w[pc];
    }
  }
  const float shB = a.shB[m];
  const float loB = a.reluB ? 0.f : -__builtin_inff();
  const int Ho = a.H / 2, Wo = a.W / 2;

  // phase A bookkeeping (tile-invariant): byte offset of this lane's pixel of each of the wave's groups in an input tile, and of
  // the 8 bytes it writes in a window tile (-1: a padding row of the last group, which repeats a real pixel and stores nothing)
  int ain[GPW], aout[GPW];
#pragma unroll
  for (int s = 0; s < GPW; ++s) {
    const int li = 16 * (p + 4 * s) + m;
    const int lc = li < NPA ? li : NPA - 1;
    const int r = lc / WS, c = lc - r * WS;
    ain[s] = (r * IWX + c) * 16;
    aout[s] = li < NPA ? (r * WST + c) * 32 + (((ksub >> 1) ^ (r & 1)) * 16) + (ksub & 1) * 8 : -1;
  }
  // phase B bookkeeping (tile-invariant): MFMA row m = position m & 3 of pool window m >> 2 of the group; the lane's pixel of
  // the wave's left group in a window tile, and per block its tap with the channel half it reads (swapped in odd window rows)
  const int pr = (m >> 1) & 1;
  const int bin = ((2 * p + pr) * WST + 2 * (m >> 2) + (m & 1)) * 32;
  int toffB[5];
#pragma unroll
  for (int blk = 0; blk < 5; ++blk) {
    const int tap = 2 * blk + (ksub >> 1) < 9 ? 2 * blk + (ksub >> 1) : 8;
    const int ky = tap / 3, kx = tap - 3 * ky;
    toffB[blk] = (ky * WST + kx) * 32 + (((ksub & 1) ^ ((pr + ky) & 1)) * 16);
  }

  const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(a.x), 0, a.bytes_x, 0x00020000);
  f32x4 pre[NIT];
  auto fetch = [&](int T) {
    const int fb = T / per, fr = T - fb * per;
    const int fy0 = (fr / tiles_x) * TSY - 2, fx0 = (fr % tiles_x) * TS - 2;
#pragma unroll
    for (int i = 0; i < NIT; ++i) {
      const int e = tid + 256 * i, cg = e & 1, pix = e >> 1;
      const int r = pix / IWX, c = pix - r * IWX;
      const int Y = fy0 + r, X = fx0 + c;
      const bool ok = (e < NPI * 2) & (Y >= 0) & (Y < a.H) & (X >= 0) & (X < a.W);
      const int off = ok ? (((fb * a.H + Y) * a.W + X) * CINA + 4 * cg) * 4 : 0x7fffffff;
      pre[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rx, off, 0, 0));
    }
  };

  const P16Walk tw = p16_tile_walk(ntiles, a.xcd_map);
  int tile = tw.first, tnext = 0;
  const int t_end = dyn ? ntiles : tw.end;  // drawn tiles come from the pool of the XCD the workgroup is ON (not blockIdx % 8's chunk)
  if (dyn) {
    tk.begin(tk_sh);
    tile = tk.cur >= 0 ? tk.cur : t_end;
  }
  if (tile < t_end) fetch(tile);
  RA_PHASE_DECL;
  for (; tile < t_end; tile = tnext) {
    const int b = tile / per, trem = tile - b * per;
    const int ty = trem / tiles_x, tx = trem - ty * tiles_x;
    // No barrier here: the input tiles were last read in phase A, before the previous tile's middle barrier, and the window tiles
    // are written only after the staging barrier below, which every wave reaches with its phase B behind it.
    RA_PHASE_AT(0);  // top of the tile
#pragma unroll
    for (int i = 0; i < NIT; ++i) {
      const int e = tid + 256 * i, cg = e & 1, pix = e >> 1;
      unsigned H0, M0, L0, H1, M1, L1;  // channels 4 cg .. 4 cg + 3 of the pixel: 8 bytes of its record in each of the three tiles
      split3_pair(pre[i].x, pre[i].y, H0, M0, L0);
      split3_pair(pre[i].z, pre[i].w, H1, M1, L1);
      if (e < NPI * 2) {
        unsigned char *rec = tinp + pix * 16 + cg * 8;
        *reinterpret_cast<u32x2 *>(rec) = u32x2{H0, H1};
        *reinterpret_cast<u32x2 *>(rec + PLI) = u32x2{M0, M1};
        *reinterpret_cast<u32x2 *>(rec + 2 * PLI) = u32x2{L0, L1};
      }
    }
    if (dyn) tk.publish(tk_sh);
    __syncthreads();
    RA_PHASE_AT(1);  // staged (split into three bf16 tiles) + barrier
    if (dyn) {
      tk.read_next(tk_sh);
      tk.request();  // older than the prefetch loads below: consumed with them at the next tile's staging
      tk.step();
      tnext = tk.cur >= 0 ? tk.cur : t_end;
    } else {
      tnext = tile + tw.step;
    }
    if (tnext < t_end) fetch(tnext);

    // ---------------- phase A: layer A on the window, BN + ReLU, -> three bf16 window tiles ----------------
    {
      const int oyA = ty * TSY - 1, oxA = tx * TS - 1;  // image coordinates of window pixel (0, 0)
      const bool interior = (oyA >= 0) & (oyA + AWY <= a.H) & (oxA >= 0) & (oxA + WS <= a.W);
      f32x4 acc[GPW];
#pragma unroll
      for (int s = 0; s < GPW; ++s) acc[s] = shA4;
      const int t0 = ksub, t1 = 4 + ksub, t2 = 8;  // this lane's tap of the three blocks (block 2: tap 8; its other k-slots carry zero weights)
      const int toff[3] = {((t0 / 3) * IWX + t0 % 3) * 16, ((t1 / 3) * IWX + t1 % 3) * 16, ((t2 / 3) * IWX + t2 % 3) * 16};
      constexpr int PA[6] = {1, 0, 2, 0, 1, 0}, PB[6] = {1, 2, 0, 1, 0, 0};  // six piece products, smallest first
#pragma unroll
      for (int blk = 0; blk < 3; ++blk)
#pragma unroll
        for (int s = 0; s < GPW; ++s) {
          s16x8 av[3];
#pragma unroll
          for (int pc = 0; pc < 3; ++pc) av[pc] = *reinterpret_cast<const s16x8 *>(tinp + ain[s] + toff[blk] + pc * PLI);
#pragma unroll
          for (int t = 0; t < 6; ++t)
            acc[s] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, wA[blk][PB[t]]), __builtin_bit_cast(bf16x8, av[PA[t]]),
                                                             acc[s], 0, 0, 0);
        }
      RA_PHASE_AT(2);  // layer A's MFMAs
#pragma unroll
      for (int s = 0; s < GPW; ++s) {
        f32x4 o = acc[s];  // D^T column m of the group = window pixel 16 g + m; rows 4 ksub + j = its channels
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = fmaxf(o[j], loA);
        if (!interior) {  // outside the image the intermediate is layer B's SAME padding: zero
          const int li = 16 * (p + 4 * s) + m;
          const int wr = li / WS, wc = li - wr * WS;
          const int Y = oyA + wr, X = oxA + wc;
          const bool ok = (Y >= 0) & (Y < a.H) & (X >= 0) & (X < a.W);
#pragma unroll
          for (int j = 0; j < 4; ++j) o[j] = ok ? o[j] : 0.f;
        }
        unsigned H01, M01, L01, H23, M23, L23;
        split3_pair(o[0], o[1], H01, M01, L01);
        split3_pair(o[2], o[3], H23, M23, L23);
        if (aout[s] >= 0) {
          unsigned char *d = twin + aout[s];
          *reinterpret_cast<u32x2 *>(d) = u32x2{H01, H23};
          *reinterpret_cast<u32x2 *>(d + PLW) = u32x2{M01, M23};
          *reinterpret_cast<u32x2 *>(d + 2 * PLW) = u32x2{L01, L23};
        }
      }
    }
    RA_PHASE_AT(3);  // layer A's epilogue -> window tiles
    __syncthreads();
    RA_PHASE_AT(4);  // barrier

    // ---------------- phase B: layer B direct out of the window tiles, max-pool in registers, -> global ----------------
    {
      f32x4 acc[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) acc[u] = f32x4{shB, shB, shB, shB};
      constexpr int PA[6] = {1, 0, 2, 0, 1, 0}, PB[6] = {1, 2, 0, 1, 0, 0};  // six piece products, smallest first
#pragma unroll
      for (int blk = 0; blk < 5; ++blk) {
        s16x8 av[2][3], wB[3];
#pragma unroll
        for (int pc = 0; pc < 3; ++pc) wB[pc] = *reinterpret_cast<const s16x8 *>(twb + ((blk * 3 + pc) * 64 + lane) * 16);
#pragma unroll
        for (int u = 0; u < 2; ++u)  // the wave's right group starts 8 window pixels further
#pragma unroll
          for (int pc = 0; pc < 3; ++pc) av[u][pc] = *reinterpret_cast<const s16x8 *>(twin + bin + u * 8 * 32 + toffB[blk] + pc * PLW);
#pragma unroll
        for (int t = 0; t < 6; ++t)
#pragma unroll
          for (int u = 0; u < 2; ++u)  // consecutive MFMAs alternate between the two groups' accumulators
            acc[u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, av[u][PA[t]]), __builtin_bit_cast(bf16x8, wB[PB[t]]),
                                                             acc[u], 0, 0, 0);
      }
      RA_PHASE_AT(5);  // layer B's MFMAs
      // D: column m = output channel, rows 4 ksub .. 4 ksub + 3 = the four pixels of pool window ksub of the group
      const int oty = ty * (TSY / 2) + p;
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const float best = fmaxf(fmaxf(fmaxf(acc[u][0], acc[u][1]), fmaxf(acc[u][2], acc[u][3])), loB);
        const int otx = tx * (TS / 2) + 4 * u + ksub;
        a.y[((size_t)(b * Ho + oty) * Wo + otx) * 16 + m] = best;
      }
      RA_PHASE_AT(6);  // pooled and stored
    }
  }
  RA_PHASE_END;
}

int launch_pair16(const P16Args &a, hipStream_t st, int *plan) {
  auto kern = conv_pair16_mfma;
  static const int resident = wgs_per_cu(kern, P16_LDS) * cu_count();
  static const int wgs = env_int("RA_PAIR16_WGS", 0);  // > 0: tuning aid, the persistent grid
  static const int cap = wgs > 0 ? wgs : resident;
  const int tiles_x = a.W / P16_TS, tiles_y = a.H / P16_TSY, ntiles = tiles_x * tiles_y * a.B;
  const int grid = ntiles < cap ? ntiles : cap;
  P16Args a2 = a;
  a2.xcd_map = (grid % 8 == 0 && grid >= 8) ? 1 : 0;
  const bool draws = ntiles >= 2 * kTicketMinTilesPerWg * grid;  // as the Winograd pair: tiles are drawn from 6 per workgroup
  if (plan) {  // ra_conv_pair16_plan
    plan[RA_PLAN_FAMILY] = RA_PLAN_FAMILY_PAIR, plan[RA_PLAN_FORM] = RA_PLAN_FORM_SPLIT | RA_PLAN_FORM_PERSIST;
    plan[RA_PLAN_CK] = 8, plan[RA_PLAN_CMID] = 16, plan[RA_PLAN_NC] = 1, plan[RA_PLAN_KF] = 3, plan[RA_PLAN_POOL] = 2, plan[RA_PLAN_SLICES] = 1;
    plan[RA_PLAN_TILE_H] = P16_TSY, plan[RA_PLAN_TILE_W] = P16_TS, plan[RA_PLAN_TILES_X] = tiles_x, plan[RA_PLAN_TILES_Y] = tiles_y;
    plan[RA_PLAN_TICKETS] = draws ? 1 : 0;
    plan_walk(plan, ntiles, grid, a2.xcd_map);
    return 0;
  }
  a2.tickets = draws ? take_ticket_slots(1, grid) : nullptr;
  hipLaunchKernelGGL(kern, dim3(grid), dim3(256), P16_LDS, st, a2, tiles_x, tiles_y, ntiles);
  return launch_status("ra_conv_pair16_f32");
}

}  // namespace cpair
}  // namespace ra

using namespace ra;

extern "C" int ra_conv_pair16_supported(int Cin, int CoutA, int CoutB, int poolB, int H, int W) {
  return Cin == 8 && CoutA == 16 && CoutB == 16 && poolB == 2 && H > 0 && W > 0 && H % 16 == 0 && W % 16 == 0;
}

// plan != nullptr (ra_conv_pair16_plan): the same checks and choices, ending in a record instead of a launch
static int pair16_entry(const float *x, int B, int H, int W, const float *wpA, const float *scaleA, const float *shiftA, int reluA,
                        const float *wpB, const float *scaleB, const float *shiftB, int reluB, float *y, void *stream, int *plan) {
  if ((!plan && (!x || !wpA || !scaleA || !shiftA || !wpB || !scaleB || !shiftB || !y)) || B <= 0)
    return fail(RA_E_INVALID, "ra_conv_pair16_f32: bad argument");
  if (!ra_conv_pair16_supported(8, 16, 16, 2, H, W)) return fail(RA_E_SHAPE, "ra_conv_pair16_f32: %dx%d", H, W);
  const size_t bytes = (size_t)B * H * W * 8 * sizeof(float);
  if (bytes >= (1ull << 31)) return fail(RA_E_SHAPE, "ra_conv_pair16_f32: input exceeds 2 GiB");
  cpair::P16Args a{};
  a.x = x;
  a.wpA = wpA;
  a.scA = scaleA;
  a.shA = shiftA;
  a.wpB = wpB;
  a.scB = scaleB;
  a.shB = shiftB;
  a.y = y;
  a.B = B;
  a.H = H;
  a.W = W;
  a.CoutAP = a.CoutBP = ra_conv_cout_padded(16);
  a.reluA = reluA;
  a.reluB = reluB;
  a.bytes_x = (int)bytes;
  a.xcd_map = 0;
  return cpair::launch_pair16(a, as_stream(stream), plan);
}

extern "C" int ra_conv_pair16_f32(const float *x, int B, int H, int W, const float *wpA, const float *scaleA, const float *shiftA,
                                  int reluA, const float *wpB, const float *scaleB, const float *shiftB, int reluB, float *y,
                                  void *stream) {
  return pair16_entry(x, B, H, W, wpA, scaleA, shiftA, reluA, wpB, scaleB, shiftB, reluB, y, stream, nullptr);
}

extern "C" int ra_conv_pair16_plan(int B, int H, int W, int *plan) {
  if (!plan) return fail(RA_E_INVALID, "ra_conv_pair16_plan: bad argument");
  for (int i = 0; i < RA_PLAN_INTS; ++i) plan[i] = 0;
  if (!plan_have_device()) return fail(RA_E_INVALID, "ra_conv_pair16_plan: the grid follows the device's CU count and occupancy: no device");
  return pair16_entry(nullptr, B, H, W, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, 0, nullptr, nullptr, plan);
}
