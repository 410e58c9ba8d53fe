// The wide filter gradient: ra_wgrad.hip's job for the layers K1-wide (ra_conv_wide.hip) runs, Cout 129 .. 512 and Cin up to 1024
// (fg_model.py:112-160 through nnlib.cnn / nnlib.dcnn, trained by fg_model.py:249-265).  For the SAME conv that ran,
//   dW[ky][kx][ci][co] = sum over b, y, x of X[b, y + ky - 1, x + kx - 1, ci] dU[b, y, x, co],   db[co] = sum dU,
// X zero-padded and, with upsample, zero-stuffed at the odd positions (the stride-2 transposed conv).
//
// GEMM view, per tap: D[ci, co] = sum_k A[ci, k] B[k, co], k = pixel.  M = Cin and N = Cout are large and K = B H W is short (256 ..
// 16 384), the opposite of ra_wgrad.hip's layers, so the kernel is OUTPUT-STATIONARY:
//   workgroup = 4 waves, owns the 64 ci x 64 co block of all 9 taps (grid.x = ci blocks, grid.y = co blocks, ragged last ones);
//   wave (wm, wn) owns 32 ci x 32 co = 2 x 2 MFMA tiles per tap: 36 independent accumulators, 144 registers, exact float32 on
//   v_mfma_f32_16x16x4_f32;
//   it walks 8 x 8 pixel tiles: per tile LDS holds the 10 x 10 halo of x as [pixel][ci 64] and the tile of dU as [pixel][co 64], rows
//   of 80 floats (two k rows of 16 lanes land on disjoint halves of the 32 banks of a ds_read_b32).  A k-step is 4 consecutive
//   pixels of a tile row; its dU operand is shared by the 9 taps, only the x operand moves with the tap: 20 LDS reads feed 36 MFMAs.
//   grid.z = the K split: part s walks the pixel tiles [s per, (s + 1) per) and writes ONE partial block [tap][ci][co] (padded
//   to the blocks) into the workspace; the chooser (wide_plan, the one place) picks the split so that the launch has about one
//   workgroup per CU and a part has at least 4 tiles.
//   The finishing pass adds the parts in order 0, 1, ... and adds the total to gw in the reference layout (through LDS for a
//   transposed filter, so that both sides are coalesced); db comes from the column sums the ci-block-0 workgroups take in LDS.
// No atomics, every sum in a fixed order: two runs give the same bits.  All offsets are size_t.
#include "ra_common.h"

namespace ra {
namespace wgw {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int TS = 8;               // pixel tile side
constexpr int LS = TS + 2;          // with halo
constexpr int MB = 64, NB = 64;     // ci / co per workgroup
constexpr int LD = 80;              // LDS row, floats: 64 channels + 16 (bank spread of the k rows)
constexpr int XA = LS * LS * LD;    // 8000
constexpr int UB = TS * TS * LD;    // 5120
constexpr int LDS_BYTES = (XA + UB) * 4;
constexpr int MAX_SPLIT = 64;
constexpr int MIN_TILES = 4;        // pixel tiles per part, at least (where there are that many)
constexpr int TARGET_WGS = 256;     // one workgroup per CU of an MI355X: the plan is a host decision and does not ask the device

struct Args {
  const float *x, *du;
  float *ws;
  int Cin, Cout, Hs, Ws, H, W, ups, tiles_x, tiles_y, ntiles, per, CinP, CoutP, split;
};

__global__ __launch_bounds__(256) void wgrad_wide(const Args a) {
  __shared__ __attribute__((aligned(16))) float lds[XA + UB];
  float *lx = lds, *lu = lds + XA;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
  const int m = lane & 15, ksub = lane >> 4;
  const int ci0 = blockIdx.x * MB, co0 = blockIdx.y * NB, part = blockIdx.z;
  const int t_begin = part * a.per, t_end = t_begin + a.per < a.ntiles ? t_begin + a.per : a.ntiles;

  f32x4 acc[9][2][2];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[t][i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  float dbsum = 0.f;
  const int aoff = ksub * LD + wm * 32 + m, boff = ksub * LD + wn * 32 + m;

  for (int t = t_begin; t < t_end; ++t) {
    int r = t;
    const int tx = r % a.tiles_x;
    r /= a.tiles_x;
    const int ty = r % a.tiles_y, b = r / a.tiles_y;
    const int y0 = ty * TS, x0 = tx * TS;
    __syncthreads();  // the previous tile's reads are done
    // ---- x: halo pixel hp = r * LS + c, channel quad q of this ci block
    for (int e = tid; e < LS * LS * (MB / 4); e += 256) {
      const int hp = e >> 4, q = e & 15, hr = hp / LS, hc = hp - hr * LS;
      int yy = y0 + hr - 1, xx = x0 + hc - 1;
      bool ok = yy >= 0 && yy < a.H && xx >= 0 && xx < a.W;
      if (a.ups) {  // zero-stuffed U[2 i + 1, 2 j + 1] = x[i, j]
        ok = ok && (yy & 1) && (xx & 1);
        yy >>= 1;
        xx >>= 1;
      }
      const int cc = ci0 + 4 * q;
      f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
      if (ok && cc < a.Cin) v = *reinterpret_cast<const f32x4 *>(a.x + (((size_t)b * a.Hs + yy) * a.Ws + xx) * a.Cin + cc);
      *reinterpret_cast<f32x4 *>(lx + hp * LD + 4 * q) = v;
    }
    // ---- dU: pixel p of the tile, channel quad q of this co block; zero outside the map, so that x's halo there adds nothing
    for (int e = tid; e < TS * TS * (NB / 4); e += 256) {
      const int p = e >> 4, q = e & 15, yy = y0 + (p >> 3), xx = x0 + (p & 7), cc = co0 + 4 * q;
      f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
      if (yy < a.H && xx < a.W && cc < a.Cout) v = *reinterpret_cast<const f32x4 *>(a.du + (((size_t)b * a.H + yy) * a.W + xx) * a.Cout + cc);
      *reinterpret_cast<f32x4 *>(lu + p * LD + 4 * q) = v;
    }
    __syncthreads();
    if (blockIdx.x == 0 && tid < NB) {  // db: this tile's column sums, pixel order
      float s = 0.f;
#pragma unroll 8
      for (int p = 0; p < TS * TS; ++p) s += lu[p * LD + tid];
      dbsum += s;
    }
#pragma unroll 2
    for (int ks = 0; ks < 16; ++ks) {  // pixels 4 ks .. 4 ks + 3: row ks / 2, columns 4 (ks % 2) ..
      const float *pu = lu + ks * 4 * LD + boff;
      const float *px = lx + ((ks >> 1) * LS + (ks & 1) * 4) * LD + aoff;
      const float b0 = pu[0], b1 = pu[16];
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) {
        const int ky = tap / 3, kx = tap % 3;
        const float a0 = px[(ky * LS + kx) * LD], a1 = px[(ky * LS + kx) * LD + 16];
        acc[tap][0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, acc[tap][0][0], 0, 0, 0);
        acc[tap][0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b1, acc[tap][0][1], 0, 0, 0);
        acc[tap][1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b0, acc[tap][1][0], 0, 0, 0);
        acc[tap][1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, acc[tap][1][1], 0, 0, 0);
      }
    }
  }

  // ---- this part's block: D register r of a lane = ci row 4 (lane >> 4) + r, co column lane & 15
  float *wp = a.ws + (size_t)part * 9 * a.CinP * a.CoutP;
#pragma unroll
  for (int tap = 0; tap < 9; ++tap)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int ci = ci0 + wm * 32 + i * 16 + 4 * ksub + r, co = co0 + wn * 32 + j * 16 + m;
          wp[((size_t)tap * a.CinP + ci) * a.CoutP + co] = acc[tap][i][j][r];
        }
  if (blockIdx.x == 0 && tid < NB) a.ws[(size_t)a.split * 9 * a.CinP * a.CoutP + (size_t)part * a.CoutP + co0 + tid] = dbsum;
}

// gw += the parts' sum, in the reference layout of the filter that ran: [3,3,cin_w,Cout], or [3,3,Cout,cin_w] with the taps
// flipped; chan_map sends a kernel channel to its filter row (-1: padding).  One writer per element.  A workgroup owns 32 ci x
// 32 co of one tap (blockIdx.z = tap; 9 = the bias sums): it reads along co, and writes a transposed filter along ci through LDS.
__global__ __launch_bounds__(256) void wgrad_wide_final(const float *ws, int split, int CinP, int CoutP, int Cin, int Cout,
                                                        const int *chan_map, int cin_w, int transposed, float *gw, float *gb) {
  __shared__ float tile[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5, cob = blockIdx.x * 32, cib = blockIdx.y * 32, tap = blockIdx.z;
  const size_t part_floats = (size_t)9 * CinP * CoutP;
  if (tap == 9) {
    const int co = cob + tx;
    if (blockIdx.y != 0 || ty != 0 || !gb || co >= Cout) return;
    float s = 0.f;
    for (int k = 0; k < split; ++k) s += ws[(size_t)split * part_floats + (size_t)k * CoutP + co];
    gb[co] += s;
    return;
  }
  const int ky = tap / 3, kx = tap - 3 * ky;
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) {
    const int ci = cib + ty + 8 * rr, co = cob + tx;
    float s = 0.f;
    if (ci < Cin && co < Cout) {
      const float *p = ws + ((size_t)tap * CinP + ci) * CoutP + co;
      for (int k = 0; k < split; ++k) s += p[(size_t)k * part_floats];
      if (!transposed) {
        const int j = chan_map ? chan_map[ci] : (ci < cin_w ? ci : -1);
        if (j >= 0) gw[((size_t)tap * cin_w + j) * Cout + co] += s;
      }
    }
    tile[ty + 8 * rr][tx] = s;
  }
  if (!transposed) return;
  __syncthreads();
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) {
    const int co = cob + ty + 8 * rr, ci = cib + tx;
    if (ci >= Cin || co >= Cout) continue;
    const int j = chan_map ? chan_map[ci] : (ci < cin_w ? ci : -1);
    if (j >= 0) gw[((size_t)((2 - ky) * 3 + (2 - kx)) * Cout + co) * cin_w + j] += tile[tx][ty + 8 * rr];
  }
}

// The one chooser: the launch of a shape in the kernel's range.  H, W: the conv's map.
struct Plan {
  int gx, gy, split, per, ntiles, tiles_x, tiles_y, CinP, CoutP;
  size_t ws_floats() const { return (size_t)split * ((size_t)9 * CinP * CoutP + CoutP); }
};
inline Plan wide_plan(int Cin, int Cout, int B, int H, int W) {
  Plan p;
  p.gx = ceil_div(Cin, MB), p.gy = ceil_div(Cout, NB);
  p.CinP = p.gx * MB, p.CoutP = p.gy * NB;
  p.tiles_x = ceil_div(W, TS), p.tiles_y = ceil_div(H, TS);
  p.ntiles = p.tiles_x * p.tiles_y * B;
  int s = ceil_div(TARGET_WGS, p.gx * p.gy);
  if (s > p.ntiles / MIN_TILES) s = p.ntiles / MIN_TILES;
  if (s > MAX_SPLIT) s = MAX_SPLIT;
  if (s < 1) s = 1;
  p.per = ceil_div(p.ntiles, s);
  p.split = ceil_div(p.ntiles, p.per);  // no empty part; the last one may be short
  return p;
}
inline bool shape_ok(int Cin, int Cout, int B, int H, int W) {
  return ra_conv_wide_supported(Cin, Cout) && B > 0 && H > 0 && W > 0 &&
         (size_t)ceil_div(W, TS) * ceil_div(H, TS) * (size_t)B < (1ull << 31);
}

}  // namespace wgw
}  // namespace ra

using namespace ra;

extern "C" int ra_conv3x3_wgrad_wide_plan(int Cin, int Cout, int B, int H, int W, int upsample, int *rec) {
  if (!rec || B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return fail(RA_E_INVALID, "ra_conv3x3_wgrad_wide_plan: bad argument");
  const int u = upsample ? 2 : 1;
  if (!wgw::shape_ok(Cin, Cout, B, H * u, W * u))
    return fail(RA_E_SHAPE, "ra_conv3x3_wgrad_wide_plan: Cin %d (%% 4, <= 1024) or Cout %d (129 .. 512, %% 16)", Cin, Cout);
  const wgw::Plan p = wgw::wide_plan(Cin, Cout, B, H * u, W * u);
  rec[RA_WGW_PLAN_TILE_CI] = wgw::MB, rec[RA_WGW_PLAN_TILE_CO] = wgw::NB, rec[RA_WGW_PLAN_TILE_PIX] = wgw::TS, rec[RA_WGW_PLAN_TAPS] = 9;
  rec[RA_WGW_PLAN_GRID_CI] = p.gx, rec[RA_WGW_PLAN_GRID_CO] = p.gy, rec[RA_WGW_PLAN_SPLIT] = p.split;
  rec[RA_WGW_PLAN_TILES_PER_PART] = p.per, rec[RA_WGW_PLAN_NTILES] = p.ntiles, rec[RA_WGW_PLAN_LDS] = wgw::LDS_BYTES;
  rec[RA_WGW_PLAN_WS_FLOATS] = (int)p.ws_floats();  // at most 64 * (9 * 1024 * 512 + 512) < 2^31
  return 0;
}

extern "C" size_t ra_conv3x3_wgrad_wide_workspace_floats(int Cin, int Cout, int B, int H, int W) {
  if (!wgw::shape_ok(Cin, Cout, B, H, W)) return 0;
  return wgw::wide_plan(Cin, Cout, B, H, W).ws_floats();
}

extern "C" int ra_conv3x3_wgrad_wide_acc_f32(const float *x, int Cin, int B, int Hs, int Ws, int upsample, const float *du, int Cout,
                                             float *ws, size_t ws_floats, const int *chan_map, int cin_w, int transposed, float *gw,
                                             float *gb, void *stream) {
  if (!x || !du || !ws || !gw || B <= 0 || Hs <= 0 || Ws <= 0 || Cin <= 0 || Cout <= 0)
    return fail(RA_E_INVALID, "ra_conv3x3_wgrad_wide_acc_f32: bad argument");
  if (cin_w <= 0 || (!chan_map && cin_w > Cin)) return fail(RA_E_INVALID, "ra_conv3x3_wgrad_wide_acc_f32: cin_w %d", cin_w);
  const int ups = upsample ? 1 : 0, H = Hs * (1 + ups), W = Ws * (1 + ups);
  if (!wgw::shape_ok(Cin, Cout, B, H, W))
    return fail(RA_E_SHAPE, "ra_conv3x3_wgrad_wide_acc_f32: Cin %d (%% 4, <= 1024) or Cout %d (129 .. 512, %% 16)", Cin, Cout);
  const wgw::Plan p = wgw::wide_plan(Cin, Cout, B, H, W);
  if (ws_floats < p.ws_floats()) return fail(RA_E_WORKSPACE, "ra_conv3x3_wgrad_wide_acc_f32: workspace too small");
  wgw::Args a;
  a.x = x, a.du = du, a.ws = ws;
  a.Cin = Cin, a.Cout = Cout, a.Hs = Hs, a.Ws = Ws, a.H = H, a.W = W, a.ups = ups;
  a.tiles_x = p.tiles_x, a.tiles_y = p.tiles_y, a.ntiles = p.ntiles, a.per = p.per, a.CinP = p.CinP, a.CoutP = p.CoutP, a.split = p.split;
  hipLaunchKernelGGL(wgw::wgrad_wide, dim3(p.gx, p.gy, p.split), dim3(256), 0, as_stream(stream), a);
  hipLaunchKernelGGL(wgw::wgrad_wide_final, dim3(ceil_div(Cout, 32), ceil_div(Cin, 32), 10), dim3(256), 0, as_stream(stream), ws, p.split,
                     p.CinP, p.CoutP, Cin, Cout, chan_map, cin_w, transposed ? 1 : 0, gw, gb);
  return launch_status("ra_conv3x3_wgrad_wide_acc_f32");
}
