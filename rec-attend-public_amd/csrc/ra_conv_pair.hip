// K1 (pair form) — TWO consecutive 3x3 SAME conv layers fused in one launch:
//   A: conv3x3 (+bias+BN+ReLU, no pool; optionally the zero-stuffed stride-2 transposed conv)
//   B: conv3x3 (+bias+BN+ReLU, max-pool 1|2)
// The A output of a tile (+1-pixel halo, recomputed) never leaves LDS, which removes the
// HBM write+read of the intermediate activation — the dominant cost of the first controller-CNN
// layers (L0 writes 8 MiB per 512x512 image that L1 reads straight back) — and halves the number
// of launches of the patch-sized attention CNN / DCNN.  Same f32 MFMA implicit-GEMM machinery as
// ra_conv.hip (v_mfma_f32_16x16x4_f32, 2x2-window row mapping, [pixel][ksub][cg] LDS records
// read with one wide ds_read per tap).  nnlib.py:229-253 (cnn) / :362-400 (dcnn), two layers.
// This file: the generic pair in its one-shot and persistent kernels, ra_conv_pair_f32 and the plan query.  The N-packed
// form of the full-resolution 8-channel pairs is in ra_conv_pair8.hip; ra_conv_pair_parts.h holds what the two share.
#include <cstdlib>

#include "ra_conv_pair_parts.h"
#include "ra_split3.h"  // the vector types

namespace ra {
namespace cpair {

// The tile geometry of one instantiation, and the phases of its two kernels as pieces.  Each kernel keeps its own skeleton —
// how the input window reaches LDS and where the filters are loaded — and declares the operand arrays itself.  The pieces
// take a thread's place in its wave as the kernels compute it: wave (uniform), A-operand row m = (q, dy, dx) and k-slot
// ksub folded into lane_in / a_base, D-side column co_lane and row block qo.  Both kernels run write_record and
// phase_b_store; phase_a and phase_b_taps are the persistent kernel's alone.  Which kernel calls which piece was decided by
// compiling all instantiations and timing both builds: profiles/pair_forms.txt.
template <int CINA, int CMID, int NCB, int GX, int GYB>
struct PGeo {
  static constexpr int NCA = (CMID + 15) / 16;
  static constexpr int TWB = 8 * GX, THB = 8 * GYB, PMB = GX * GYB;
  static constexpr int GXA = GX + 1, GRA = THB / 2 + 1, NGA = GXA * GRA;
  static constexpr int AW = 8 * GXA, AH = 2 * GRA;     // A-out tile (B tile + halo, padded)
  static constexpr int LWA = AW + 2, LHA = AH + 2;     // input tile of A
  static constexpr int NCGA = CINA / 4, CKA = CINA < 16 ? CINA : 16, NCHA = CINA / CKA, NCGAC = CKA / 4;
  static constexpr int NCGB = CMID / 4, CKB = CMID < 16 ? CMID : 16, NCHB = CMID / CKB, NCGBC = CKB / 4;
  static constexpr int KSA = 9 * NCGAC, KSB = 9 * NCGBC;
  static constexpr int IN_FLOATS = LHA * LWA * CINA;
  static constexpr int MID_FLOATS = AH * AW * CMID;
  static constexpr int RA = 4;                          // A groups per wave per round
  static constexpr int GPW = (NGA + 3) / 4;             // A groups per wave
  static constexpr int ROUNDS = (GPW + RA - 1) / RA;
  typedef typename vec_of<NCGAC>::type avecA;
  typedef typename vec_of<NCGBC>::type avecB;

  // one input pixel's channels v[cg] = channels 4 cg .. 4 cg + 3 -> its LDS record [ksub][cg]
  __device__ __forceinline__ static void write_record(float *rec, const f32x4 (&v)[NCGA]) {
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      if constexpr (NCGA == 1) {
        rec[ks] = v[0][ks];
      } else if constexpr (NCGA == 2) {
        rec[ks * 2] = v[0][ks];
        rec[ks * 2 + 1] = v[1][ks];
      } else {
#pragma unroll
        for (int c4 = 0; c4 < NCGA / 4; ++c4)
          *reinterpret_cast<f32x4 *>(rec + ks * NCGA + 4 * c4) =
              f32x4{v[4 * c4][ks], v[4 * c4 + 1][ks], v[4 * c4 + 2][ks], v[4 * c4 + 3][ks]};
      }
    }
  }

  // phase A: conv A over the B tile + halo out of tin, result -> tmid.  The persistent kernel's, as is phase_b_taps below: the
  // one-shot kernel keeps its own copies of the two MFMA loops (with the calls, two of its instantiations lose a resident
  // workgroup per CU and one runs 2.4 % slower: profiles/pair_forms.txt).  A fix to either loop is made in both places.
  __device__ __forceinline__ static void phase_a(const PArgs &a, int wave, int lane_in, int co_lane, int qo, int ty0, int tx0,
                                                 const float *tin, float *tmid, const float (&scA)[NCA], const float (&shA)[NCA],
                                                 const float (&bregA)[KSA][NCA]) {
    for (int rd = 0; rd < ROUNDS; ++rd) {
      f32x4 acc[RA][NCA];
      int gbase[RA], gr[RA], gc[RA];
#pragma unroll
      for (int j = 0; j < RA; ++j) {
        int gi = wave + 4 * (rd * RA + j);
        if (gi >= NGA) gi = NGA - 1;  // duplicate work, masked at the store
        gr[j] = gi / GXA;
        gc[j] = gi % GXA;
        gbase[j] = (2 * gr[j] * LWA + 8 * gc[j]) * CINA + lane_in;
#pragma unroll
        for (int n = 0; n < NCA; ++n) acc[j][n] = f32x4{0.f, 0.f, 0.f, 0.f};
      }
      for (int ch = 0; ch < NCHA; ++ch) {
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
          const int ky = tap / 3, kx = tap % 3;
          avecA av[RA];
#pragma unroll
          for (int j = 0; j < RA; ++j)
            av[j] = *reinterpret_cast<const avecA *>(&tin[gbase[j] + (ky * LWA + kx) * CINA + ch * NCGAC]);
#pragma unroll
          for (int cg = 0; cg < NCGAC; ++cg)
#pragma unroll
            for (int j = 0; j < RA; ++j)
#pragma unroll
              for (int n = 0; n < NCA; ++n)
                acc[j][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j][cg], bregA[tap * NCGAC + cg][n], acc[j][n], 0, 0, 0);
        }
      }
      // A epilogue -> tmid (zero outside the image: it is B's SAME padding).  Tiles whose whole
      // A region lies inside the image (uniform test) skip the per-value bounds arithmetic.
      const bool interior = (ty0 >= 1) & (ty0 - 1 + AH <= a.H) & (tx0 >= 1) & (tx0 + TWB + 1 <= a.W);
      const float loA = a.reluA ? 0.f : -__builtin_inff();
#pragma unroll
      for (int j = 0; j < RA; ++j) {
        const bool live = (wave + 4 * (rd * RA + j)) < NGA;
#pragma unroll
        for (int n = 0; n < NCA; ++n) {
          const int co = 16 * n + co_lane;
          float o[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) o[r] = fmaxf(acc[j][n][r] * scA[n] + shA[n], loA);
          if (!interior) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int Y = ty0 - 1 + 2 * gr[j] + (r >> 1), X = tx0 - 1 + 8 * gc[j] + 2 * qo + (r & 1);
              o[r] = ((Y >= 0) & (Y < a.H) & (X >= 0) & (X < a.W)) ? o[r] : 0.f;
            }
          }
          if (live && co < CMID) {
            float *dst = tmid + ((2 * gr[j]) * AW + 8 * gc[j] + 2 * qo) * CMID + (co & 3) * NCGB + (co >> 2);
#pragma unroll
            for (int r = 0; r < 4; ++r) dst[((r >> 1) * AW + (r & 1)) * CMID] = o[r];
          }
        }
      }
    }
  }

  // phase B, the nine taps of intermediate-channel chunk ch out of tmid: acc += A(tmid) x bregB
  __device__ __forceinline__ static void phase_b_taps(const float *tmid, int a_base, int ch, const float (&bregB)[KSB][NCB],
                                                      f32x4 (&acc)[PMB][NCB]) {
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int ky = tap / 3, kx = tap % 3;
      avecB av[PMB];
#pragma unroll
      for (int g = 0; g < PMB; ++g) {
        const int gx = g % GX, gy = g / GX;
        av[g] = *reinterpret_cast<const avecB *>(&tmid[a_base + ((2 * gy + ky) * AW + 8 * gx + kx) * CMID + ch * NCGBC]);
      }
#pragma unroll
      for (int cg = 0; cg < NCGBC; ++cg)
#pragma unroll
        for (int g = 0; g < PMB; ++g)
#pragma unroll
          for (int n = 0; n < NCB; ++n)
            acc[g][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[g][cg], bregB[tap * NCGBC + cg][n], acc[g][n], 0, 0, 0);
    }
  }

  // phase B epilogue: BN + ReLU (+ 2x2 max-pool) of the tile at (b, ty0, tx0) -> global, ragged tiles masked per value
  __device__ __forceinline__ static void phase_b_store(const PArgs &a, int wave, int co_lane, int qo, int b, int ty0, int tx0,
                                                       const f32x4 (&acc)[PMB][NCB]) {
    const int opool = a.poolB;
    const float loB = a.reluB ? 0.f : -__builtin_inff();
    const int wrow0 = ty0 + wave * 2 * GYB, lcol0 = tx0 + 2 * qo;
#pragma unroll
    for (int n = 0; n < NCB; ++n) {
      const int co = 16 * n + co_lane;
      const float sc = a.scB[co], sh = a.shB[co];
      const bool co_ok = co < a.CoutB;
      const int obase = ((b * a.Ho + wrow0 / opool) * a.Wo + lcol0 / opool) * a.CoutB + co;
#pragma unroll
      for (int g = 0; g < PMB; ++g) {
        const int gx = g % GX, gy = g / GX;
        const int row0 = wrow0 + 2 * gy, col0 = lcol0 + 8 * gx;
        float v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = fmaxf(acc[g][n][r] * sc + sh, loB);
        if (opool == 2) {
          const float o = fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3]));
          if (co_ok && (row0 >> 1) < a.Ho && (col0 >> 1) < a.Wo)
            a.y[obase + (gy * a.Wo + 4 * gx) * a.CoutB] = o;
        } else {
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (co_ok && row0 + (r >> 1) < a.Ho && col0 + (r & 1) < a.Wo)
              a.y[obase + ((2 * gy + (r >> 1)) * a.Wo + 8 * gx + (r & 1)) * a.CoutB] = v[r];
        }
      }
    }
  }
};

// One tile per workgroup: the input window staged straight from global memory (zero-stuffed for the transposed conv, the canvas
// plane patched in), the filters loaded per channel chunk inside the phases.
template <int CINA, int CMID, int NCB, int GX, int GYB>
__global__ __launch_bounds__(256) void conv_pair_mfma(const PArgs a, int tiles_x, int tiles_y) {
  using G = PGeo<CINA, CMID, NCB, GX, GYB>;
  constexpr int NCA = G::NCA;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float *tin = lds;                  // [LHA][LWA][CINA]  records [ksub][cg]
  float *tmid = lds + G::IN_FLOATS;  // [AH][AW][CMID]    records [ksub][cg]
  typedef typename G::avecA avecA;
  typedef typename G::avecB avecB;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // wave-uniform: group bookkeeping on the SALU
  const int m = lane & 15, ksub = lane >> 4;
  const int q = m >> 2, dy = (m >> 1) & 1, dx = m & 1;
  const int co_lane = lane & 15, qo = lane >> 4;
  const int per = tiles_x * tiles_y;
  const int b = blockIdx.x / per;
  const int trem = blockIdx.x - b * per;
  const int ty0 = (trem / tiles_x) * G::THB, tx0 = (trem % tiles_x) * G::TWB;

  // ---------------- phase 0: stage A's input tile (+2-pixel halo) ----------------
  {
    const int sy0 = a.ups ? (ty0 >> 1) : ty0, sx0 = a.ups ? (tx0 >> 1) : tx0;
    const float *base = a.src + ((size_t)(b * a.Hs + sy0) * a.Ws + sx0) * a.C0;
    for (int e = tid; e < G::LHA * G::LWA; e += 256) {
      const int rr = e / G::LWA - 2, cc = e % G::LWA - 2;  // relative to the B-tile origin
      const int Y = ty0 + rr, X = tx0 + cc;
      bool ok = (Y >= 0) & (Y < a.H) & (X >= 0) & (X < a.W);
      int ys = rr, xs = cc;
      if (a.ups) {
        ok = ok & (rr & 1) & (cc & 1);  // origins are even: parity of Y == parity of rr
        ys = rr >> 1;
        xs = cc >> 1;
      }
      f32x4 v[G::NCGA];
#pragma unroll
      for (int cg = 0; cg < G::NCGA; ++cg) {
        v[cg] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (ok) v[cg] = *reinterpret_cast<const f32x4 *>(base + (ys * a.Ws + xs) * a.C0 + 4 * cg);
      }
      if (a.plane && ok) {
        const float pv = a.plane[(size_t)(b * a.Hs + sy0 + ys) * a.Ws + sx0 + xs];
        const int pg = a.plane_chan >> 2, slot = a.plane_chan & 3;
#pragma unroll
        for (int cg = 0; cg < G::NCGA; ++cg) {  // selects, not runtime register indexing
          v[cg].x = (cg == pg && slot == 0) ? pv : v[cg].x;
          v[cg].y = (cg == pg && slot == 1) ? pv : v[cg].y;
          v[cg].z = (cg == pg && slot == 2) ? pv : v[cg].z;
          v[cg].w = (cg == pg && slot == 3) ? pv : v[cg].w;
        }
      }
      G::write_record(tin + e * CINA, v);
    }
  }
  __syncthreads();

  // ---------------- phase A: conv A over the B tile + halo, result -> LDS ----------------
  {
    float scA[NCA], shA[NCA];
#pragma unroll
    for (int n = 0; n < NCA; ++n) {
      scA[n] = a.scA[16 * n + co_lane];
      shA[n] = a.shA[16 * n + co_lane];
    }
    const int lane_in = (dy * G::LWA + 2 * q + dx) * CINA + ksub * G::NCGA;
    float bregA[G::KSA][NCA];
    auto load_bA = [&](int ch) {
      const float *wrow = a.wpA + ((size_t)ch * G::KSA * 4 + ksub) * a.CoutAP + co_lane;
#pragma unroll
      for (int s = 0; s < G::KSA; ++s)
#pragma unroll
        for (int n = 0; n < NCA; ++n) bregA[s][n] = wrow[(size_t)s * 4 * a.CoutAP + 16 * n];
    };
    if (G::NCHA == 1) load_bA(0);
    // (PGeo::phase_a, in place)
    for (int rd = 0; rd < G::ROUNDS; ++rd) {
      f32x4 acc[G::RA][NCA];
      int gbase[G::RA], gr[G::RA], gc[G::RA];
#pragma unroll
      for (int j = 0; j < G::RA; ++j) {
        int gi = wave + 4 * (rd * G::RA + j);
        if (gi >= G::NGA) gi = G::NGA - 1;  // duplicate work, masked at the store
        gr[j] = gi / G::GXA;
        gc[j] = gi % G::GXA;
        gbase[j] = (2 * gr[j] * G::LWA + 8 * gc[j]) * CINA + lane_in;
#pragma unroll
        for (int n = 0; n < NCA; ++n) acc[j][n] = f32x4{0.f, 0.f, 0.f, 0.f};
      }
      for (int ch = 0; ch < G::NCHA; ++ch) {
        if (G::NCHA > 1) load_bA(ch);
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
          const int ky = tap / 3, kx = tap % 3;
          avecA av[G::RA];
#pragma unroll
          for (int j = 0; j < G::RA; ++j)
            av[j] = *reinterpret_cast<const avecA *>(
                &tin[gbase[j] + (ky * G::LWA + kx) * CINA + ch * G::NCGAC]);
#pragma unroll
          for (int cg = 0; cg < G::NCGAC; ++cg)
#pragma unroll
            for (int j = 0; j < G::RA; ++j)
#pragma unroll
              for (int n = 0; n < NCA; ++n)
                acc[j][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j][cg], bregA[tap * G::NCGAC + cg][n],
                                                                 acc[j][n], 0, 0, 0);
        }
      }
      // A epilogue -> tmid (zero outside the image: it is B's SAME padding).  Tiles whose whole
      // A region lies inside the image (uniform test) skip the per-value bounds arithmetic.
      const bool interior = (ty0 >= 1) & (ty0 - 1 + G::AH <= a.H) & (tx0 >= 1) & (tx0 + G::TWB + 1 <= a.W);
      const float loA = a.reluA ? 0.f : -__builtin_inff();
#pragma unroll
      for (int j = 0; j < G::RA; ++j) {
        const bool live = (wave + 4 * (rd * G::RA + j)) < G::NGA;
#pragma unroll
        for (int n = 0; n < NCA; ++n) {
          const int co = 16 * n + co_lane;
          float o[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) o[r] = fmaxf(acc[j][n][r] * scA[n] + shA[n], loA);
          if (!interior) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int Y = ty0 - 1 + 2 * gr[j] + (r >> 1), X = tx0 - 1 + 8 * gc[j] + 2 * qo + (r & 1);
              o[r] = ((Y >= 0) & (Y < a.H) & (X >= 0) & (X < a.W)) ? o[r] : 0.f;
            }
          }
          if (live && co < CMID) {
            float *dst = tmid + ((2 * gr[j]) * G::AW + 8 * gc[j] + 2 * qo) * CMID + (co & 3) * G::NCGB + (co >> 2);
#pragma unroll
            for (int r = 0; r < 4; ++r) dst[((r >> 1) * G::AW + (r & 1)) * CMID] = o[r];
          }
        }
      }
    }
  }
  __syncthreads();

  // ---------------- phase B: conv B out of tmid, epilogue -> global ----------------
  {
    f32x4 acc[G::PMB][NCB];
#pragma unroll
    for (int g = 0; g < G::PMB; ++g)
#pragma unroll
      for (int n = 0; n < NCB; ++n) acc[g][n] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int a_base = ((wave * 2 * GYB + dy) * G::AW + 2 * q + dx) * CMID + ksub * G::NCGB;
    float bregB[G::KSB][NCB];
    for (int ch = 0; ch < G::NCHB; ++ch) {
      {
        const float *wrow = a.wpB + ((size_t)ch * G::KSB * 4 + ksub) * a.CoutBP + co_lane;
#pragma unroll
        for (int s = 0; s < G::KSB; ++s)
#pragma unroll
          for (int n = 0; n < NCB; ++n) bregB[s][n] = wrow[(size_t)s * 4 * a.CoutBP + 16 * n];
      }
      // (PGeo::phase_b_taps, in place)
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) {
        const int ky = tap / 3, kx = tap % 3;
        avecB av[G::PMB];
#pragma unroll
        for (int g = 0; g < G::PMB; ++g) {
          const int gx = g % GX, gy = g / GX;
          av[g] = *reinterpret_cast<const avecB *>(
              &tmid[a_base + ((2 * gy + ky) * G::AW + 8 * gx + kx) * CMID + ch * G::NCGBC]);
        }
#pragma unroll
        for (int cg = 0; cg < G::NCGBC; ++cg)
#pragma unroll
          for (int g = 0; g < G::PMB; ++g)
#pragma unroll
            for (int n = 0; n < NCB; ++n)
              acc[g][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[g][cg], bregB[tap * G::NCGBC + cg][n],
                                                               acc[g][n], 0, 0, 0);
      }
    }
    G::phase_b_store(a, wave, co_lane, qo, b, ty0, tx0, acc);
  }
}

// Persistent workgroups over the tiles of plain single-chunk pairs: both layers' filters loaded once per workgroup, the next
// tile's input window fetched into registers behind the MFMA phases.
template <int CINA, int CMID, int NCB, int GX, int GYB>
__global__ __launch_bounds__(256) void conv_pair_persist_mfma(const PArgs a, int tiles_x, int tiles_y, int ntiles) {
  using G = PGeo<CINA, CMID, NCB, GX, GYB>;
  constexpr int NCA = G::NCA;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float *tin = lds;                  // [LHA][LWA][CINA]  records [ksub][cg]
  float *tmid = lds + G::IN_FLOATS;  // [AH][AW][CMID]    records [ksub][cg]

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // wave-uniform: group bookkeeping on the SALU
  const int m = lane & 15, ksub = lane >> 4;
  const int q = m >> 2, dy = (m >> 1) & 1, dx = m & 1;
  const int co_lane = lane & 15, qo = lane >> 4;
  const int per = tiles_x * tiles_y;
  static_assert(G::NCHA == 1 && G::NCHB == 1, "persistent pair: single-chunk layers");
  // both layers' B operands and epilogue constants: once per workgroup
  float scA[NCA], shA[NCA];
#pragma unroll
  for (int n = 0; n < NCA; ++n) {
    scA[n] = a.scA[16 * n + co_lane];
    shA[n] = a.shA[16 * n + co_lane];
  }
  float bregA[G::KSA][NCA], bregB[G::KSB][NCB];
  {
    const float *wrow = a.wpA + (size_t)ksub * a.CoutAP + co_lane;
#pragma unroll
    for (int s = 0; s < G::KSA; ++s)
#pragma unroll
      for (int n = 0; n < NCA; ++n) bregA[s][n] = wrow[(size_t)s * 4 * a.CoutAP + 16 * n];
    const float *wrowb = a.wpB + (size_t)ksub * a.CoutBP + co_lane;
#pragma unroll
    for (int s = 0; s < G::KSB; ++s)
#pragma unroll
      for (int n = 0; n < NCB; ++n) bregB[s][n] = wrowb[(size_t)s * 4 * a.CoutBP + 16 * n];
  }
  // the input window (tile + 2-pixel halo) of a tile is fetched into registers one tile ahead
  constexpr int NPIXA = G::LHA * G::LWA, NIT = (NPIXA + 255) / 256;
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(a.src), 0, a.bytes0, 0x00020000);
  int e_r[NIT], e_c[NIT];
#pragma unroll
  for (int i = 0; i < NIT; ++i) {
    const int e = tid + 256 * i;
    e_r[i] = e / G::LWA - 2;
    e_c[i] = e % G::LWA - 2;
    if (e >= NPIXA) e_r[i] = -(1 << 20);
  }
  f32x4 pre[NIT][G::NCGA];
  auto fetch = [&](int T) {
    const int fb = T / per, fr = T - fb * per;
    const int fy0 = (fr / tiles_x) * G::THB, fx0 = (fr % tiles_x) * G::TWB;
#pragma unroll
    for (int i = 0; i < NIT; ++i) {
      const int Y = fy0 + e_r[i], X = fx0 + e_c[i];
      const bool ok = (Y >= 0) & (Y < a.H) & (X >= 0) & (X < a.W);
      const int off = ok ? (((fb * a.Hs + Y) * a.Ws + X) * a.C0) * 4 : 0x7fffffff;
#pragma unroll
      for (int cg = 0; cg < G::NCGA; ++cg)
        pre[i][cg] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, off, 16 * cg, 0));
    }
  };
  int tile = blockIdx.x;
  if (tile < ntiles) fetch(tile);
  for (; tile < ntiles; tile += gridDim.x) {
    const int b = tile / per;
    const int trem = tile - b * per;
    const int ty0 = (trem / tiles_x) * G::THB, tx0 = (trem % tiles_x) * G::TWB;

    // ---------------- phase 0: prefetched registers -> LDS (previous tile's phase B is complete
    // for every wave once all have arrived at the barrier below) ----------------
#pragma unroll
    for (int i = 0; i < NIT; ++i) {
      const int e = tid + 256 * i;
      if (e < NPIXA) G::write_record(tin + e * CINA, pre[i]);
    }
    __syncthreads();
    {
      const int next = tile + gridDim.x;
      if (next < ntiles) fetch(next);  // in flight across both MFMA phases
    }

    // ---------------- phase A: conv A over the B tile + halo, result -> LDS ----------------
    {
      const int lane_in = (dy * G::LWA + 2 * q + dx) * CINA + ksub * G::NCGA;
      G::phase_a(a, wave, lane_in, co_lane, qo, ty0, tx0, tin, tmid, scA, shA, bregA);
    }
    __syncthreads();

    // ---------------- phase B: conv B out of tmid, epilogue -> global ----------------
    {
      f32x4 acc[G::PMB][NCB];
#pragma unroll
      for (int g = 0; g < G::PMB; ++g)
#pragma unroll
        for (int n = 0; n < NCB; ++n) acc[g][n] = f32x4{0.f, 0.f, 0.f, 0.f};
      const int a_base = ((wave * 2 * GYB + dy) * G::AW + 2 * q + dx) * CMID + ksub * G::NCGB;
      G::phase_b_taps(tmid, a_base, 0, bregB, acc);
      G::phase_b_store(a, wave, co_lane, qo, b, ty0, tx0, acc);
    }
  }
}

template <int CINA, int CMID, int NCB, int GX, int GYB>
int launch(const PArgs &a, int B, hipStream_t st, int *plan) {
  using G = PGeo<CINA, CMID, NCB, GX, GYB>;
  auto kern = conv_pair_mfma<CINA, CMID, NCB, GX, GYB>;
  constexpr size_t lds = (size_t)(G::IN_FLOATS + G::MID_FLOATS) * sizeof(float);
  static_assert(lds <= 160 * 1024, "pair tile does not fit LDS");
  const int tiles_x = ceil_div(a.W, G::TWB), tiles_y = ceil_div(a.H, G::THB);
  const int ntiles = tiles_x * tiles_y * B;
  if (plan) {  // ra_conv_pair_plan: the geometry is a function of the shape; whether the persistent kernel runs needs the device
    plan[RA_PLAN_FAMILY] = RA_PLAN_FAMILY_PAIR;
    plan[RA_PLAN_CK] = CINA, plan[RA_PLAN_CMID] = CMID, plan[RA_PLAN_NC] = NCB, plan[RA_PLAN_GX] = GX, plan[RA_PLAN_GY] = GYB;
    plan[RA_PLAN_KF] = 3, plan[RA_PLAN_TILE_H] = G::THB, plan[RA_PLAN_TILE_W] = G::TWB;
    plan[RA_PLAN_TILES_X] = tiles_x, plan[RA_PLAN_TILES_Y] = tiles_y, plan[RA_PLAN_NTILES] = ntiles;
    plan[RA_PLAN_GRID] = ntiles, plan[RA_PLAN_TILES_MIN] = plan[RA_PLAN_TILES_MAX] = 1;
    if (!(G::NCHA == 1 && G::NCHB == 1) || a.ups || a.plane) return 0;  // never the persistent kernel
    if (!plan_have_device()) {
      plan[RA_PLAN_GRID] = plan[RA_PLAN_TILES_MIN] = plan[RA_PLAN_TILES_MAX] = -1;
      return 0;
    }
  } else {
    static const MaxDynamicLds lds_limit(kern, lds);
  }
  if constexpr (G::NCHA == 1 && G::NCHB == 1) {
    // plain single-chunk pairs (controller CNN L2+L3 at full size): persistent workgroups, weights
    // loaded once, the next tile's input prefetched into registers behind the MFMA phases
    static const int pers = env_int("RA_PAIR_PERSIST", 1);
    static const int cap = wgs_per_cu(conv_pair_persist_mfma<CINA, CMID, NCB, GX, GYB>, lds) * cu_count();
    if (pers && !a.ups && !a.plane && ntiles > cap && a.bytes0 > 0) {
      if (plan) {
        plan[RA_PLAN_FORM] = RA_PLAN_FORM_PERSIST;
        plan_walk(plan, ntiles, cap, 0);
        return 0;
      }
      hipLaunchKernelGGL((conv_pair_persist_mfma<CINA, CMID, NCB, GX, GYB>), dim3(cap), dim3(256), lds, st, a, tiles_x,
                         tiles_y, ntiles);
      return launch_status("ra_conv_pair_f32");
    }
  }
  if (plan) return 0;
  hipLaunchKernelGGL(kern, dim3(ntiles), dim3(256), lds, st, a, tiles_x, tiles_y);
  return launch_status("ra_conv_pair_f32");
}

template <int CINA, int CMID, int NCB>
int dispatch_geo(const PArgs &a, int B, hipStream_t st, int *plan) {
  using Big = PGeo<CINA, CMID, NCB, 4, 2>;
  constexpr bool big_fits = (size_t)(Big::IN_FLOATS + Big::MID_FLOATS) * 4 <= 80 * 1024;
  const bool narrow = (a.W % 32 != 0) && (a.W % 32 <= 16);
  auto wgs = [&](int gx, int gyb) { return (long)ceil_div(a.W, 8 * gx) * ceil_div(a.H, 8 * gyb) * B; };
  static const int force = env_int("RA_PAIR_GEO", 0);  // =<gx><gyb>: tuning aid
  // single-chunk plain pairs run the persistent kernel, which measures fastest with the 8-row tile
  // (cfg2 L2+L3: 41.8 us at 32x8 against 47.4 at 32x16 and 45.3 one-shot; profiles/r02)
  constexpr bool single_chunk = Big::NCHA == 1 && Big::NCHB == 1;
  if (!force && single_chunk && !a.ups && !a.plane && !narrow && wgs(4, 1) >= 2048)
    return launch<CINA, CMID, NCB, 4, 1>(a, B, st, plan);
  if constexpr (big_fits) {
    if (force == 42 || (!force && !narrow && wgs(4, 2) >= 512)) return launch<CINA, CMID, NCB, 4, 2>(a, B, st, plan);
  }
  if (force == 41 || (!force && !narrow)) return launch<CINA, CMID, NCB, 4, 1>(a, B, st, plan);
  if (force == 22 || (!force && wgs(2, 2) >= 512)) return launch<CINA, CMID, NCB, 2, 2>(a, B, st, plan);
  return launch<CINA, CMID, NCB, 2, 1>(a, B, st, plan);
}

template <int CINA, int CMID>
int dispatch_b(const PArgs &a, int B, hipStream_t st, int *plan) {
  if (a.CoutBP == 16) return dispatch_geo<CINA, CMID, 1>(a, B, st, plan);
  if (a.CoutBP == 32) return dispatch_geo<CINA, CMID, 2>(a, B, st, plan);
  return fail(RA_E_SHAPE, "ra_conv_pair_f32: CoutB %d unsupported", a.CoutB);
}

template <int CINA>
int dispatch_mid(const PArgs &a, int cmid, int B, hipStream_t st, int *plan) {
  switch (cmid) {
    case 8: return dispatch_b<CINA, 8>(a, B, st, plan);
    case 16: return dispatch_b<CINA, 16>(a, B, st, plan);
    case 32: return dispatch_b<CINA, 32>(a, B, st, plan);
    default: return fail(RA_E_SHAPE, "ra_conv_pair_f32: CoutA %d unsupported", cmid);
  }
}

}  // namespace cpair
}  // namespace ra

using namespace ra;

extern "C" int ra_conv_pair_supported(int Cin, int CoutA, int CoutB) {
  const bool cin_ok = Cin == 4 || Cin == 8 || Cin == 16 || Cin == 32;
  const bool mid_ok = CoutA == 8 || CoutA == 16 || CoutA == 32;
  return cin_ok && mid_ok && CoutB >= 1 && CoutB <= 32;
}

// plan != nullptr (ra_conv_pair_plan): the same checks and choices, ending in a record instead of a launch; `plane` is then a mere
// non-null mark and no pointer is followed
static int pair_entry(const float *src, int Cin, int B, int Hs, int Ws, int upsampleA, const float *wpA, const float *scaleA,
                      const float *shiftA, int CoutA, int reluA, const float *wpB, const float *scaleB, const float *shiftB,
                      int CoutB, int reluB, int poolB, const float *plane, int plane_chan, float *y, void *stream, int *plan) {
  if (cpair::missing_pointer(plan, {src, wpA, scaleA, shiftA, wpB, scaleB, shiftB, y}) || B <= 0 || Hs <= 0 || Ws <= 0)
    return fail(RA_E_INVALID, "ra_conv_pair_f32: bad argument");
  if (!ra_conv_pair_supported(Cin, CoutA, CoutB))
    return fail(RA_E_SHAPE, "ra_conv_pair_f32: Cin=%d CoutA=%d CoutB=%d", Cin, CoutA, CoutB);
  if (poolB != 1 && poolB != 2) return fail(RA_E_SHAPE, "ra_conv_pair_f32: pool %d", poolB);
  cpair::PArgs a = cpair::pair_args(src, Cin, B, Hs, Ws, upsampleA, wpA, scaleA, shiftA, CoutA, reluA, wpB, scaleB, shiftB, CoutB, reluB,
                                    poolB, plane, plane_chan, y);
  if (poolB == 2 && ((a.H | a.W) & 1)) return fail(RA_E_SHAPE, "ra_conv_pair_f32: odd size with pool 2");
  if (plane && (plane_chan < 0 || plane_chan >= Cin)) return fail(RA_E_INVALID, "ra_conv_pair_f32: plane channel");
  hipStream_t st = as_stream(stream);
  const size_t bytes0 = (size_t)B * Hs * Ws * Cin * 4;
  a.bytes0 = (int)bytes0;
  static int no8 = -1;  // RA_PAIR_NO8=1: tuning aid, disables the N-packed kernel
  if (no8 < 0) no8 = getenv("RA_PAIR_NO8") ? 1 : 0;
  if (!no8 && (Cin == 4 || Cin == 8) && CoutA == 8 && CoutB <= 8 && poolB == 2 && !a.ups && bytes0 < (1u << 31) && a.W > 16)
    return cpair::launch_npacked(a, B, st, plan);
  switch (Cin) {
    case 4: return cpair::dispatch_mid<4>(a, CoutA, B, st, plan);
    case 8: return cpair::dispatch_mid<8>(a, CoutA, B, st, plan);
    case 16: return cpair::dispatch_mid<16>(a, CoutA, B, st, plan);
    default: return cpair::dispatch_mid<32>(a, CoutA, B, st, plan);
  }
}

extern "C" int ra_conv_pair_f32(const float *src, int Cin, int B, int Hs, int Ws, int upsampleA,
                                const float *wpA, const float *scaleA, const float *shiftA, int CoutA,
                                int reluA, const float *wpB, const float *scaleB, const float *shiftB,
                                int CoutB, int reluB, int poolB, const float *plane, int plane_chan,
                                float *y, void *stream) {
  return pair_entry(src, Cin, B, Hs, Ws, upsampleA, wpA, scaleA, shiftA, CoutA, reluA, wpB, scaleB, shiftB, CoutB, reluB, poolB, plane,
                    plane_chan, y, stream, nullptr);
}

extern "C" int ra_conv_pair_plan(int Cin, int B, int Hs, int Ws, int upsampleA, int CoutA, int CoutB, int poolB, int has_plane,
                                 int cache_form, int *plan) {
  if (!plan) return fail(RA_E_INVALID, "ra_conv_pair_plan: bad argument");
  for (int i = 0; i < RA_PLAN_INTS; ++i) plan[i] = 0;
  static float mark;  // never read or written: a non-null stand-in for the canvas plane
  if (cache_form == 1)
    return cpair::fill_cache_entry(nullptr, &mark, 3, B, Hs, Ws, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, CoutB, 0, nullptr, nullptr,
                                   nullptr, 0, 0.0f, nullptr, plan);
  if (cache_form == 2)
    return cpair::cached_entry(nullptr, &mark, 3, B, Hs, Ws, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, CoutB, 0, nullptr, nullptr, plan);
  if (cache_form) return fail(RA_E_INVALID, "ra_conv_pair_plan: cache_form %d", cache_form);
  return pair_entry(nullptr, Cin, B, Hs, Ws, upsampleA, nullptr, nullptr, nullptr, CoutA, 0, nullptr, nullptr, nullptr, CoutB, 0, poolB,
                    has_plane ? &mark : nullptr, has_plane ? 0 : -1, nullptr, nullptr, plan);
}
