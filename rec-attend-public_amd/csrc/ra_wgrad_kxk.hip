// =================================================================================================
// KF x KF conv backward-weight on the f32 MFMA, KF in {1, 5, 7} (nnlib.cnn / nnlib.dcnn layers of another filter size:
// nnlib.py:131-257, :260-404).  For the SAME conv u = conv(X, Wf) that ra_convkxk_f32 ran, the kernel returns
//   dWf[ky][kx][ci][co] = sum_{b,y,x} X[b, y+ky-org, x+kx-org, ci] * dU[b, y, x, co]   and   db[co] = sum dU,
// X zero-padded; org = KF / 2, or with `upsample` (X = the staged image U[2i+1] = x[i] of a stride-2 transposed conv) the
// forward's window origin KF - 2 - max(KF - 2, 0) / 2: -1, 2, 3 for KF = 1, 5, 7.
// Same GEMM view as ra_wgrad.hip (D[ci, co] = sum_pixels A[ci, pixel] B[pixel, co], the pixels are K of
// v_mfma_f32_16x16x4_f32), but the taps are SPLIT OVER THE GRID: a workgroup owns one tap row ky (blockIdx.z), a 16-channel
// slice of Cin (blockIdx.y) and 16 NT output channels, and walks 8 x 32 pixel tiles persistently.  It keeps KF + 1 (the KF taps
// of the row + the bias, summed by the ky = 0 workgroups alone) x NT accumulator tiles per wave — 16 at KF = 7, NT = 2 — and
// stages only the 8 x (32 + KF - 1) pixels of x its tap row reads ([8][LW][16] floats) beside the dU tile: 51 KB at KF = 7,
// NT = 2, where the 3 x 3 kernel's scheme would hold 50 NT tiles and a [14][38][16] slice.  The four waves split the tile's
// rows (K split) and are summed through LDS in wave order; the workgroup writes ONE partial record [kx (KF = bias)][16][16 NT],
// and wgrad_kxk_final_kernel adds the records in a fixed order: no atomics, two runs give the same bits.
// The next tile's global loads travel in registers across the MFMA loop of the current one (as wgrad_kernel<PRE>).
#include "ra_common.h"

namespace ra {
namespace train {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int KTH = 8, KTW = 32;  // the pixel tile

constexpr int kxk_record_floats(int KF, int CP) { return (KF + 1) * 16 * CP; }
// dynamic LDS: x rows of the tap row + halo columns [KTH][KTW + KF - 1][16], dU tile [KTH][KTW][CP]; then ONE record
constexpr size_t kxk_lds_bytes(int KF, int CP) {
  const size_t stage = (size_t)(KTH * (KTW + KF - 1) * 16 + KTH * KTW * CP) * 4, rec = (size_t)kxk_record_floats(KF, CP) * 4;
  return stage > rec ? stage : rec;
}

template <int KF, int NT>  // NT: output channels per workgroup / 16; blockIdx.z = slice * KF + ky
__global__ __launch_bounds__(256) void wgrad_kxk_kernel(const float *x, const float *du, int Hs, int Ws, int Cin, int ups, int org,
                                                        int H, int W, int Cout, int tiles_x, int tiles_y, int ntiles, float *part) {
  constexpr int CP = 16 * NT, LW = KTW + KF - 1;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float *tx = lds;                   // [KTH][LW][16]  the rows y + ky - org of the input slice, channel-contiguous
  float *tu = lds + KTH * LW * 16;   // [KTH][KTW][CP] output-gradient tile
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m = lane & 15, ksub = lane >> 4;
  const int slice = blockIdx.z / KF, ky = blockIdx.z - slice * KF;
  const int co0 = slice * CP, c0 = blockIdx.y * 16;
  const int cn = Cin - c0 < 16 ? Cin - c0 : 16, ng = (cn + 3) >> 2;  // real channels of the slice, in groups of 4
  f32x4 acc[KF + 1][NT];
#pragma unroll
  for (int t = 0; t <= KF; ++t)
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[t][n] = f32x4{0.f, 0.f, 0.f, 0.f};
  const bool vec_du = (Cout & 3) == 0;
  const int per = tiles_x * tiles_y;
  // The NEXT tile's global loads are issued into registers before the MFMA loop of the current one and written to LDS after it
  // (one staging buffer, two barriers per tile): every load unconditional (clamped address, value selected afterwards), so all
  // of a tile's loads are in flight together and behind the matrix work.  A Cout that is no multiple of 4 (the one-channel
  // output layer) stages dU element by element at commit time instead.
  constexpr int NIX = KTH * LW * 4, NRX = (NIX + 255) / 256, NRU = KTH * KTW * (CP / 4) / 256;
  f32x4 rx[NRX], ru[NRU];
  auto prefetch = [&](int tile) {
    const int b = tile / per, tr = tile - b * per;
    const int ty0 = (tr / tiles_x) * KTH, tx0 = (tr % tiles_x) * KTW;
#pragma unroll
    for (int i = 0; i < NRX; ++i) {  // one float4 (4 channels) per item; groups beyond the slice are zero
      const int e = tid + 256 * i;
      const int pix = e >> 2, c4 = e & 3;
      const int r = pix / LW, c = pix - r * LW;
      const int Y = ty0 + r + ky - org, X = tx0 + c - org;
      bool ok = (e < NIX) & (c4 < ng) & (Y >= 0) & (Y < H) & (X >= 0) & (X < W);
      int ys = Y, xs = X;
      if (ups) {
        ok = ok & (Y & 1) & (X & 1);
        ys = (Y - 1) >> 1;
        xs = (X - 1) >> 1;
      }
      const size_t off = ok ? (((size_t)b * Hs + ys) * Ws + xs) * Cin + c0 + 4 * c4 : 0;
      const f32x4 v = *reinterpret_cast<const f32x4 *>(x + off);
      rx[i] = ok ? v : f32x4{0.f, 0.f, 0.f, 0.f};
    }
    if (vec_du) {
#pragma unroll
      for (int i = 0; i < NRU; ++i) {  // zero beyond Cout / the image
        const int e = tid + 256 * i;
        const int c4 = e % (CP / 4), pix = e / (CP / 4);
        const int r = pix / KTW, c = pix - r * KTW;
        const int Y = ty0 + r, X = tx0 + c;
        const bool ok = (Y < H) & (X < W) & (co0 + 4 * c4 < Cout);
        const size_t off = ok ? (((size_t)b * H + Y) * W + X) * Cout + co0 + 4 * c4 : 0;
        const f32x4 v = *reinterpret_cast<const f32x4 *>(du + off);
        ru[i] = ok ? v : f32x4{0.f, 0.f, 0.f, 0.f};
      }
    }
  };
  auto commit = [&](int tile) {  // the prefetched tile -> LDS
#pragma unroll
    for (int i = 0; i < NRX; ++i) {
      const int e = tid + 256 * i;
      if (e < NIX) *reinterpret_cast<f32x4 *>(tx + (e >> 2) * 16 + 4 * (e & 3)) = rx[i];
    }
    if (vec_du) {
#pragma unroll
      for (int i = 0; i < NRU; ++i) {
        const int e = tid + 256 * i;
        *reinterpret_cast<f32x4 *>(tu + (e / (CP / 4)) * CP + 4 * (e % (CP / 4))) = ru[i];
      }
    } else {
      const int b = tile / per, tr = tile - b * per;
      const int ty0 = (tr / tiles_x) * KTH, tx0 = (tr % tiles_x) * KTW;
      for (int e = tid; e < KTH * KTW * CP; e += 256) {
        const int co = e % CP, pix = e / CP;
        const int r = pix / KTW, c = pix - r * KTW;
        const int Y = ty0 + r, X = tx0 + c;
        float v = 0.f;
        if (Y < H && X < W && co0 + co < Cout) v = du[(((size_t)b * H + Y) * W + X) * Cout + co0 + co];
        tu[e] = v;
      }
    }
  };
  if ((int)blockIdx.x < ntiles) prefetch(blockIdx.x);
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    __syncthreads();  // the previous tile's MFMA reads are complete
    commit(tile);
    __syncthreads();
    if (tile + (int)gridDim.x < ntiles) prefetch(tile + gridDim.x);  // in flight across the MFMA loop below
    // this wave's rows: 2 of the 8; K steps of 4 consecutive pixels of a row; tap kx reads the x column col + kx
#pragma unroll 1
    for (int rr = 0; rr < 2; ++rr) {
      const int row = wave * 2 + rr;
#pragma unroll 2
      for (int s = 0; s < KTW / 4; ++s) {
        const int col = 4 * s + ksub;
        float bv[NT];
#pragma unroll
        for (int n = 0; n < NT; ++n) bv[n] = tu[(row * KTW + col) * CP + 16 * n + m];
#pragma unroll
        for (int kx = 0; kx < KF; ++kx) {
          const float av = tx[(row * LW + col + kx) * 16 + m];
#pragma unroll
          for (int n = 0; n < NT; ++n) acc[kx][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv[n], acc[kx][n], 0, 0, 0);
        }
        if (ky == 0) {  // uniform: the bias belongs to the first tap row's workgroups
#pragma unroll
          for (int n = 0; n < NT; ++n) acc[KF][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(1.0f, bv[n], acc[KF][n], 0, 0, 0);
        }
      }
    }
  }
  // the 4 waves (K split) are summed through LDS in wave order, then one record per workgroup:
  // part[((slice * chunks + chunk) * KF + ky) * gridDim.x + blockIdx.x][kx (KF = bias)][16][CP]; D rows 4 * (lane >> 4) + r, column lane & 15
  __syncthreads();
  float *red = lds;
  for (int w = 0; w < 4; ++w) {
    if (wave == w) {
#pragma unroll
      for (int t = 0; t <= KF; ++t)
#pragma unroll
        for (int n = 0; n < NT; ++n)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float *d = red + (t * 16 + 4 * ksub + r) * CP + 16 * n + m;
            *d = (w == 0 ? 0.f : *d) + acc[t][n][r];
          }
    }
    __syncthreads();
  }
  constexpr int REC = kxk_record_floats(KF, CP);
  float *dst = part + ((((size_t)slice * gridDim.y + blockIdx.y) * KF + ky) * gridDim.x + blockIdx.x) * REC;
  for (int e = tid; e < REC; e += 256) dst[e] = red[e];
}

// The records -> dW and db, fixed order.  A lane owns one element of the record (64 consecutive floats per wave load), the four
// waves split the nwg records and meet in LDS as (0 + 1) + (2 + 3).  acc == 0: dw [KF,KF,Cin,Cout] and db are WRITTEN; acc == 1:
// the sums are ADDED to the filter's gradient in the reference's layout, [KF,KF,cin_w,Cout] or, transposed, [KF,KF,Cout,cin_w]
// with the taps flipped; chan_map sends a kernel channel to its filter row (-1: padding).  One writer per element.
// grid (ceil(record / 64), chunks * KF, slices).
__global__ __launch_bounds__(256) void wgrad_kxk_final_kernel(const float *part, int nwg, int nchunks, int KF, int CP, int Cin, int Cout,
                                                              const int *chan_map, int cin_w, int transposed, int acc, float *gw,
                                                              float *gb) {
  __shared__ float red[4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, rec = (KF + 1) * 16 * CP;
  const int r = blockIdx.x * 64 + lane, chunk = blockIdx.y / KF, ky = blockIdx.y - chunk * KF, slice = blockIdx.z;
  float s = 0.f;
  if (r < rec) {
    const float *p = part + (((size_t)slice * nchunks + chunk) * KF + ky) * nwg * rec + r;
    int k = wave;
    for (; k + 28 < nwg; k += 32) {  // eight loads in flight (one load per add measured ~130 us for 2 048 records)
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
  const int kx = r / (16 * CP), cl = (r / CP) & 15, cs = r % CP;
  const int ci = chunk * 16 + cl, co = slice * CP + cs;
  if (co >= Cout) return;
  if (kx == KF) {
    if (gb && ky == 0 && chunk == 0 && cl == 0) gb[co] = acc ? gb[co] + s : s;
    return;
  }
  if (ci >= Cin) return;
  if (!acc) {
    gw[((size_t)(ky * KF + kx) * Cin + ci) * Cout + co] = s;
    return;
  }
  const int j = chan_map ? chan_map[ci] : (ci < cin_w ? ci : -1);
  if (j < 0 || j >= cin_w) return;
  const size_t idx = transposed ? ((size_t)((KF - 1 - ky) * KF + (KF - 1 - kx)) * Cout + co) * cin_w + j
                                : ((size_t)(ky * KF + kx) * cin_w + j) * Cout + co;
  gw[idx] += s;
}

// ---- device-side weight repack for a KF x KF filter (the host form is ra_conv_pack_weights_k): the filter changes every step ----
__global__ __launch_bounds__(256) void pack_weights_k_kernel(const float *w, int KF, int Cin_w, int Cout, int Cin, const int *chan_map,
                                                             int tr, int CK, int cp, float *out) {
  const int KK = KF * KF, total = KK * Cin * cp, NCG = CK / 4;
  for (int e = blockIdx.x * 256 + threadIdx.x; e < total; e += gridDim.x * 256) {
    const int co = e % cp;
    int r = e / cp;
    const int ksub = r % 4;
    r /= 4;
    const int cg = r % NCG;
    r /= NCG;
    const int tap = r % KK, chunk = r / KK;
    const int c = chunk * CK + cg * 4 + ksub;
    const int src_c = chan_map ? chan_map[c] : c;
    const int ky = tap / KF, kx = tap - ky * KF;
    float v = 0.f;
    if (co < Cout && src_c >= 0 && src_c < Cin_w) {
      if (!tr)
        v = w[(((size_t)ky * KF + kx) * Cin_w + src_c) * Cout + co];
      else  // conv2d_transpose filter [KF,KF,Cout,Cin_w]: flip taps, swap in/out
        v = w[(((size_t)(KF - 1 - ky) * KF + (KF - 1 - kx)) * Cout + co) * Cin_w + src_c];
    }
    out[e] = v;
  }
}

// ---- y[b,i,j,:] = x[b,2i,2j,:]: the adjoint of a stride-2 transposed conv's zero-stuffing as a 1 x 1 filter sees it (its
// window on the stuffed image sits on the EVEN positions; the centred windows of KF = 3, 5, 7 sit on the odd ones) ----
__global__ __launch_bounds__(256) void subsample_even_kernel(const float *x, int B, int H, int W, int C, float *y) {
  const size_t total = (size_t)B * H * W * C;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
    const int c = (int)(e % C);
    size_t r = e / C;
    const int j = (int)(r % W);
    r /= W;
    const int i = (int)(r % H), b = (int)(r / H);
    y[e] = x[(((size_t)b * 2 * H + 2 * i) * 2 * W + 2 * j) * C + c];
  }
}

}  // namespace train
}  // namespace ra

using namespace ra;

namespace {

struct KxkRequest {
  const float *x = nullptr, *du = nullptr;
  int KF = 0, Cin = 0, Cout = 0, B = 0, Hs = 0, Ws = 0, upsample = 0;
  float *dw = nullptr, *db = nullptr;
  bool acc = false;
  const int *chan_map = nullptr;
  int cin_w = 0, transposed = 0;
  float *ws = nullptr;
  size_t ws_floats = 0;
  void *stream = nullptr;
  int ups() const { return upsample ? 1 : 0; }
  int H() const { return Hs * (1 + ups()); }
  int W() const { return Ws * (1 + ups()); }
  int tiles_x() const { return ceil_div(W(), train::KTW); }
  int tiles_y() const { return ceil_div(H(), train::KTH); }
  int ntiles() const { return tiles_x() * tiles_y() * B; }
};

struct KxkForm {
  int NT;        // 16 NT output channels per workgroup and record
  dim3 grid;     // (persistent workgroups, 16-channel chunks of Cin, Cout slices * KF tap rows)
  size_t lds;
  int record;    // floats of one record
  size_t ws_floats() const { return (size_t)grid.x * grid.y * grid.z * record; }
};

bool kxk_size(int KF) { return KF == 1 || KF == 5 || KF == 7; }
bool kxk_shape_ok(int KF, int Cin, int Cout) { return kxk_size(KF) && Cin > 0 && Cin % 4 == 0 && ra_conv_cout_padded(Cout) != 0; }

// The launch form of a checked shape.  NT = 2 wherever the padded Cout has 32 channels: 16 accumulator tiles at KF = 7 and 51 KB
// of LDS (three workgroups per CU).  About kTargetWgs workgroups in all whatever the layer — the tap rows, chunks and slices
// multiply them — so that the records stay small (a 128 -> 128 layer at KF = 7 has 224 of them per persistent workgroup).
KxkForm choose_kxk_form(const KxkRequest &r) {
  constexpr int kTargetWgs = 2048;
  const int cp = ra_conv_cout_padded(r.Cout), NT = cp >= 32 ? 2 : 1;
  const int chunks = ceil_div(r.Cin, 16), slices = cp / (16 * NT);
  int gx = kTargetWgs / (chunks * slices * r.KF);
  gx = gx < 1 ? 1 : gx;
  gx = gx < r.ntiles() ? gx : r.ntiles();
  return {NT, dim3(gx, chunks, slices * r.KF), train::kxk_lds_bytes(r.KF, 16 * NT), train::kxk_record_floats(r.KF, 16 * NT)};
}

template <int KF, int NT>
void launch_kxk(const KxkForm &f, const KxkRequest &r) {
  const int org = r.ups() ? KF - 2 - (KF > 2 ? KF - 2 : 0) / 2 : KF / 2;  // ra_convkxk_f32's window origin
  hipLaunchKernelGGL((train::wgrad_kxk_kernel<KF, NT>), f.grid, dim3(256), f.lds, as_stream(r.stream), r.x, r.du, r.Hs, r.Ws, r.Cin, r.ups(),
                     org, r.H(), r.W(), r.Cout, r.tiles_x(), r.tiles_y(), r.ntiles(), r.ws);
}
template <int KF>
void launch_kxk_nt(const KxkForm &f, const KxkRequest &r) {
  f.NT == 1 ? launch_kxk<KF, 1>(f, r) : launch_kxk<KF, 2>(f, r);
}

int kxk_impl(const KxkRequest &r, const char *entry) {
  if (!kxk_size(r.KF)) return fail(RA_E_SHAPE, "%s: filter size %d not built (1, 3, 5, 7)", entry, r.KF);
  if (r.Cin <= 0 || r.Cout <= 0 || r.Cin % 4 || !ra_conv_cout_padded(r.Cout)) return fail(RA_E_SHAPE, "%s: Cin %d %% 4 or Cout %d", entry, r.Cin, r.Cout);
  if (!r.x || !r.du || !r.ws || !r.dw || r.B <= 0 || r.Hs <= 0 || r.Ws <= 0) return fail(RA_E_INVALID, "%s: bad argument", entry);
  if (r.acc && (r.cin_w <= 0 || (!r.chan_map && r.cin_w > r.Cin))) return fail(RA_E_INVALID, "%s: cin_w %d", entry, r.cin_w);
  const KxkForm f = choose_kxk_form(r);
  if (r.ws_floats < f.ws_floats()) return fail(RA_E_WORKSPACE, "%s: workspace too small", entry);
  switch (r.KF) {
    case 1: launch_kxk_nt<1>(f, r); break;
    case 5: launch_kxk_nt<5>(f, r); break;
    default: launch_kxk_nt<7>(f, r); break;
  }
  const int per = 16 * f.NT, chunks = f.grid.y, slices = f.grid.z / r.KF;
  hipLaunchKernelGGL(train::wgrad_kxk_final_kernel, dim3(ceil_div(f.record, 64), chunks * r.KF, slices), dim3(256), 0, as_stream(r.stream), r.ws,
                     (int)f.grid.x, chunks, r.KF, per, r.Cin, r.Cout, r.chan_map, r.cin_w, r.transposed ? 1 : 0, r.acc ? 1 : 0, r.dw, r.db);
  return launch_status(entry);
}

}  // namespace

// H, W: the conv's map (twice x's with upsample), as ra_conv3x3_wgrad_workspace_floats takes them
extern "C" size_t ra_convkxk_wgrad_workspace_floats(int KF, int Cin, int Cout, int B, int H, int W) {
  if (KF == 3) return ra_conv3x3_wgrad_workspace_floats(Cin, Cout, B, H, W);
  if (!kxk_shape_ok(KF, Cin, Cout) || B <= 0 || H <= 0 || W <= 0) return 0;
  KxkRequest r;
  r.KF = KF; r.Cin = Cin; r.Cout = Cout; r.B = B; r.Hs = H; r.Ws = W;
  return choose_kxk_form(r).ws_floats();
}

extern "C" int ra_convkxk_wgrad_plan(int KF, int Cin, int Cout, int B, int H, int W, int *rec) {
  if (!rec) return fail(RA_E_INVALID, "ra_convkxk_wgrad_plan: bad argument");
  if (!kxk_shape_ok(KF, Cin, Cout) || B <= 0 || H <= 0 || W <= 0)
    return fail(RA_E_SHAPE, "ra_convkxk_wgrad_plan: filter size %d (1, 5, 7), Cin %d %% 4 or Cout %d", KF, Cin, Cout);
  KxkRequest r;
  r.KF = KF; r.Cin = Cin; r.Cout = Cout; r.B = B; r.Hs = H; r.Ws = W;
  const KxkForm f = choose_kxk_form(r);
  rec[RA_WGK_PLAN_NT] = f.NT, rec[RA_WGK_PLAN_GRID_X] = f.grid.x, rec[RA_WGK_PLAN_GRID_Y] = f.grid.y, rec[RA_WGK_PLAN_GRID_Z] = f.grid.z;
  rec[RA_WGK_PLAN_LDS_BYTES] = (int)f.lds, rec[RA_WGK_PLAN_RECORD_FLOATS] = f.record, rec[RA_WGK_PLAN_NTILES] = r.ntiles();
  rec[RA_WGK_PLAN_ACC_TILES] = (KF + 1) * f.NT;
  return 0;
}

extern "C" int ra_convkxk_wgrad_f32(const float *x, int Cin, int B, int Hs, int Ws, int upsample, const float *du, int Cout, int KF,
                                    float *ws, size_t ws_floats, float *dw, float *db, void *stream) {
  if (KF == 3) return ra_conv3x3_wgrad_f32(x, Cin, B, Hs, Ws, upsample, du, Cout, ws, ws_floats, dw, db, stream);
  KxkRequest r;
  r.x = x; r.du = du; r.KF = KF; r.Cin = Cin; r.Cout = Cout; r.B = B; r.Hs = Hs; r.Ws = Ws; r.upsample = upsample;
  r.ws = ws; r.ws_floats = ws_floats; r.dw = dw; r.db = db; r.stream = stream;
  return kxk_impl(r, "ra_convkxk_wgrad_f32");
}

extern "C" int ra_convkxk_wgrad_acc_f32(const float *x, int Cin, int B, int Hs, int Ws, int upsample, const float *du, int Cout, int KF,
                                        float *ws, size_t ws_floats, const int *chan_map, int Cin_w, int transposed, float *gw,
                                        float *gb, void *stream) {
  if (KF == 3)
    return ra_conv3x3_wgrad_acc_f32(x, Cin, B, Hs, Ws, upsample, du, Cout, ws, ws_floats, chan_map, Cin_w, transposed, gw, gb, stream);
  KxkRequest r;
  r.x = x; r.du = du; r.KF = KF; r.Cin = Cin; r.Cout = Cout; r.B = B; r.Hs = Hs; r.Ws = Ws; r.upsample = upsample;
  r.ws = ws; r.ws_floats = ws_floats; r.dw = gw; r.db = gb; r.stream = stream;
  r.acc = true; r.chan_map = chan_map; r.cin_w = Cin_w; r.transposed = transposed;
  return kxk_impl(r, "ra_convkxk_wgrad_acc_f32");
}

extern "C" int ra_conv_pack_weights_k_dev(const float *w, int KF, int Cin_w, int Cout, int Cin, const int *chan_map, int flags,
                                          float *out, void *stream) {
  const int cp = ra_conv_cout_padded(Cout);
  if (!w || !out || Cin_w <= 0 || Cin <= 0) return fail(RA_E_INVALID, "ra_conv_pack_weights_k_dev: bad argument");
  if (KF != 1 && KF != 3 && KF != 5 && KF != 7) return fail(RA_E_SHAPE, "ra_conv_pack_weights_k_dev: filter size %d not built (1, 3, 5, 7)", KF);
  if (Cin % 4 || !cp) return fail(RA_E_SHAPE, "ra_conv_pack_weights_k_dev: Cin %d %% 4 or Cout %d", Cin, Cout);
  if (!chan_map && Cin_w != Cin) return fail(RA_E_SHAPE, "ra_conv_pack_weights_k_dev: Cin_w != Cin without map");
  // the chunk of ra_conv_pack_weights_k: 16 / 8 / 4 (the largest dividing Cin) for KF <= 3, 8 or 4 for KF = 5, 4 for KF = 7
  const int CK = KF <= 3 ? ((Cin % 16 == 0) ? 16 : (Cin % 8 == 0) ? 8 : 4) : (KF == 5 && Cin % 8 == 0) ? 8 : 4;
  const int total = KF * KF * Cin * cp;
  hipLaunchKernelGGL(train::pack_weights_k_kernel, dim3(ceil_div(total, 256)), dim3(256), 0, as_stream(stream), w, KF, Cin_w, Cout, Cin,
                     chan_map, (flags & RA_CONV_TRANSPOSED) ? 1 : 0, CK, cp, out);
  return launch_status("ra_conv_pack_weights_k_dev");
}

extern "C" int ra_subsample_even_f32(const float *x, int B, int H, int W, int C, float *y, void *stream) {
  if (!x || !y || B <= 0 || H <= 0 || W <= 0 || C <= 0) return fail(RA_E_INVALID, "ra_subsample_even_f32: bad argument");
  size_t grid = ((size_t)B * H * W * C + 255) / 256;
  if (grid > 8192) grid = 8192;
  hipLaunchKernelGGL(train::subsample_even_kernel, dim3((unsigned)grid), dim3(256), 0, as_stream(stream), x, B, H, W, C, y);
  return launch_status("ra_subsample_even_f32");
}
