// K18 — the Cityscapes pixel-level evaluation (data_api/cityscapes_scripts/evaluation/evalPixelLevelSemanticLabeling.py,
// cited as :line): the confusion matrix of a label image against the ground truth (:566-573) and the per-instance true
// positives behind the instance-weighted iIoU (:576-615), for a label image any method wrote or for the arg-max of the
// pre-stage's semantic map, evaluated on the fly.
//
//   sem_labels   the label image of a semantic map sem [B,Hs,Ws,C] at the labels' size: every channel resized as
//                ra_instance_class.hip resizes it (resample::tap: cv2's INTER_LINEAR float path, the coordinate in double),
//                the FIRST maximum over the channels, channel 0 -> label 0 and channel c >= 1 -> gtid::cs_label_id(c - 1).
//                All channels of a pixel go through one loop body with the pixel's taps and weights, so channels that are
//                equal at the four taps give exactly equal values and the lower index wins.
//   confusion    a workgroup walks tiles of 1024 pixels of one image, 4 consecutive pixels per lane: 16 bytes of gt_ids, 4 of
//                gt_labels (or the label derived from the id), 4 of the prediction, the next tile's loads in flight under
//                the current tile's work.  The fused form has no prediction to load: thread t evaluates label_at() — the SAME
//                device function as sem_labels — for the pixels t, t + 256, ... of the tile, the order in which neighbouring
//                lanes share taps, and the 1024 labels change hands in LDS; no full-size plane is written (with the lane's
//                own 4 consecutive pixels instead, every load touched four times the cache lines and the fused form took 516
//                us where sem_labels + label form took 373).  A pixel is the cell (g, p) of a 35 x 35
//                table — index 34 collects every label above 33, so nothing is indexed by an unchecked value — and the slot
//                of its id in the catalogue (gtid::find_slot, the catalogue in LDS).  A wave's 256 consecutive pixels mostly
//                share ONE (cell, slot): the wave peels its distinct pairs one by one — the pair of the first lane that
//                still has one, four ballots, four population counts in scalar registers, and ONE LDS add per table — as the
//                overlap kernel (ra_instance_overlap.hip) does; after kPeel pairs (noise) the rest is added per run of equal
//                pairs within a lane.  The counters (35 x 35 cells, 2 x 256 instance counters: 6.9 KB) live in LDS.  Every
//                workgroup leaves them in ws, and the finishing launch adds them: per image in int32 (H * W < 2^31), over the
//                images into the int64 matrix.  No global atomics: exact, and the same on every run.
#include <cmath>
#include <cstdint>

#include "ra_common.h"
#include "ra_gt_ids.h"
#include "ra_resample.h"

namespace ra {
namespace pix {

typedef int i32x4 __attribute__((ext_vector_type(4)));
constexpr int kL = RA_PIXEL_LABELS;       // 34
constexpr int kL1 = kL + 1;               // one more row and column: labels above 33
constexpr int kCells = kL1 * kL1;         // 1225
constexpr int kMaxGt = RA_OVERLAP_MAX_GT;  // 256 catalogue slots
constexpr int kTile = RA_PIXEL_TILE;      // pixels per tile: 256 threads x 4
constexpr int kTargetWgs = 2048;          // eight workgroups per CU: a tile is a chain of latencies (loads, four searches of the
                                          // catalogue, the peel), and only other waves hide it — 8 per SIMD is what the CU holds
constexpr int kPeel = 6;                  // distinct (cell, slot) pairs a wave peels per tile before it adds per lane
constexpr int kMinC = 2, kMaxC = 9;       // channels of the semantic map: background + up to the eight thing labels
constexpr int kItp = kCells, kIctp = kCells + kMaxGt, kFlag = kCells + 2 * kMaxGt;  // a workgroup's record in ws
constexpr int kRec = 1740;                // kFlag + 1, rounded up to 16 bytes
constexpr int kFinCols = 16;              // finishing launch: entries of the record per workgroup, 256 / 16 slices of partials
constexpr int kConfJobs = (kCells + kFinCols - 1) / kFinCols;  // 77
constexpr int kInstJobs = 2 * kMaxGt / kFinCols;               // 32 per image

struct SemSrc {
  const float *sem;
  int Hs, Ws, C;
  double sy, sx;
};

// The label of pixel (r, c) of the H x W image behind the semantic map semb [Hs,Ws,C] of one image.
__device__ __forceinline__ int label_at(const float *semb, int Hs, int Ws, int C, double sy, double sx, int r, int c) {
  const int arg = resample::argmax_channel_at(semb, Hs, Ws, C, sy, sx, r, c);
  return arg == 0 ? 0 : gtid::cs_label_id(arg - 1);  // arg - 1 < kMaxC - 1 = kCsClasses
}

// One thread per output pixel.
__global__ __launch_bounds__(256) void sem_labels_kernel(SemSrc s, unsigned HW, int W, unsigned char *labels) {
  const int b = blockIdx.y;
  const unsigned e = blockIdx.x * 256u + threadIdx.x;
  if (e >= HW) return;
  const int r = (int)(e / (unsigned)W), c = (int)(e - (unsigned)r * (unsigned)W);
  labels[(size_t)b * HW + e] = (unsigned char)label_at(s.sem + (size_t)b * s.Hs * s.Ws * s.C, s.Hs, s.Ws, s.C, s.sy, s.sx, r, c);
}

__device__ __forceinline__ int clamp_label(int v) { return (unsigned)v < (unsigned)kL ? v : kL; }

// n pixels of the pair ck = cell | (slot + 1) << 11 into the workgroup's counters
__device__ __forceinline__ void add_pair(int *cnt, int *itp, int *ictp, const int *cat, int ck, int n) {
  const int cell = ck & 2047, s = (ck >> 11) - 1;  // cell < kCells, s < kMaxGt: both made from checked values
  atomicAdd(&cnt[cell], n);
  if (s < 0) return;
  const int p = cell % kL1, lab = cat[s] / 1000;  // :583, :591: the instance's label, whatever gt_labels says
  if (p < kL && p == lab) atomicAdd(&itp[s], n);
  const int cl = gtid::cs_instance_category(lab);
  if (cl != 0 && gtid::cs_instance_category(p) == cl) atomicAdd(&ictp[s], n);  // :579, :606
}

// Workgroup (x, b) walks the tiles x, x + gridDim.x, ... of image b; see the head of the file.  SEM: the prediction is
// label_at() of src.sem, else the label image pred.  VEC: 16- and 4-byte loads (H * W % 4 == 0 and the pointers aligned), else
// element loads.  Its counters go to part[b][x][kRec].
template <bool SEM, bool VEC>
__global__ __launch_bounds__(256) void confusion_kernel(const unsigned char *pred, SemSrc src, const int *gt,
                                                         const unsigned char *gl, const int *ids, const int *count,
                                                         unsigned HW, int W, int ntiles, int *part) {
  __shared__ int cnt[kCells], itp[kMaxGt], ictp[kMaxGt], cat[kMaxGt], flag[1];
  __shared__ __attribute__((aligned(4))) unsigned char labs[SEM ? kTile : 4];  // SEM: the tile's labels
  const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
  int n = count[b];
  n = n < 0 ? 0 : (n > kMaxGt ? kMaxGt : n);
  for (int i = tid; i < kCells; i += 256) cnt[i] = 0;
  itp[tid] = 0, ictp[tid] = 0;
  cat[tid] = tid < n ? ids[(size_t)b * kMaxGt + tid] : 0x7fffffff;
  if (tid == 0) flag[0] = 0;
  __syncthreads();
  const int *g = gt + (size_t)b * HW;
  const unsigned char *glb = gl ? gl + (size_t)b * HW : nullptr;
  const unsigned char *pb = SEM ? nullptr : pred + (size_t)b * HW;
  const float *semb = SEM ? src.sem + (size_t)b * src.Hs * src.Ws * src.C : nullptr;

  // this lane's 16 bytes of gt_ids and 4 bytes of gt_labels / pred of a tile
  const auto load_tile = [&](int tile, i32x4 &id, unsigned &lw, unsigned &pw) {
    const unsigned base = (unsigned)tile * kTile + 4 * tid;  // < 2^31 + kTile
    id = i32x4{-1, -1, -1, -1};
    lw = 0, pw = 0;
    if (VEC) {  // base < HW implies base + 3 < HW
      if (base < HW) {
        id = *reinterpret_cast<const i32x4 *>(g + base);
        if (glb) lw = *reinterpret_cast<const unsigned *>(glb + base);
        if (!SEM) pw = *reinterpret_cast<const unsigned *>(pb + base);
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (base + j < HW) {
          id[j] = g[base + j];
          if (glb) lw |= (unsigned)glb[base + j] << (8 * j);
          if (!SEM) pw |= (unsigned)pb[base + j] << (8 * j);
        }
    }
  };
  i32x4 id_next;
  unsigned lw_next, pw_next;
  if ((int)blockIdx.x < ntiles) load_tile(blockIdx.x, id_next, lw_next, pw_next);
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const unsigned base = (unsigned)tile * kTile + 4 * tid;
    bool ok[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) ok[j] = base + j < HW;  // still to be counted
    const i32x4 id = id_next;
    const unsigned lw = lw_next;
    unsigned pw = pw_next;
    if (tile + (int)gridDim.x < ntiles) load_tile(tile + gridDim.x, id_next, lw_next, pw_next);  // in flight under this tile's work
    if (SEM) {
      // thread t evaluates the pixels t, t + 256, ... of the tile: neighbouring lanes share taps, a quarter of the cache lines
      // per load of the lane-owns-4-pixels order; the labels change hands in LDS
      __syncthreads();  // the previous tile's labels have been read
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const unsigned e = (unsigned)tile * kTile + j * 256 + tid;
        int lab = 0;
        if (e < HW) {
          const int r = (int)(e / (unsigned)W), c = (int)(e - (unsigned)r * (unsigned)W);
          lab = label_at(semb, src.Hs, src.Ws, src.C, src.sy, src.sx, r, c);
        }
        labs[j * 256 + tid] = (unsigned char)lab;
      }
      __syncthreads();
      pw = *reinterpret_cast<const unsigned *>(&labs[4 * tid]);
    }
    int ck[4], prev_slot = -1;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int gl_j = glb ? (int)((lw >> (8 * j)) & 255u) : (id[j] < 0 ? kL : gtid::cs_label_of_id(id[j]));
      const int cell = clamp_label(gl_j) * kL1 + clamp_label((int)((pw >> (8 * j)) & 255u));
      const int s = !ok[j] ? -1 : (j > 0 && id[j] == id[j - 1] ? prev_slot : gtid::find_slot(cat, n, id[j]));
      prev_slot = s;
      ck[j] = cell | (s + 1) << 11;
    }
    // the wave's distinct pairs, one by one
    for (int it = 0; it < kPeel; ++it) {
      const bool mine = ok[0] || ok[1] || ok[2] || ok[3];
      const unsigned long long left = __ballot(mine);
      if (!left) break;
      const int srcl = __ffsll((long long)left) - 1;
      const int cand = ok[0] ? ck[0] : ok[1] ? ck[1] : ok[2] ? ck[2] : ck[3];
      const int k = __shfl(cand, srcl, 64);  // uniform
      int tot = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool hit = ok[j] && ck[j] == k;
        tot += __popcll(__ballot(hit));
        ok[j] = ok[j] && !hit;
      }
      if (lane == 0) add_pair(cnt, itp, ictp, cat, k, tot);
    }
    // what is left after kPeel pairs: per lane, per run of equal pairs
    int c = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (ok[j]) {
        ++c;
        if (j == 3 || !ok[j + 1] || ck[j + 1] != ck[j]) {
          add_pair(cnt, itp, ictp, cat, ck[j], c);
          c = 0;
        }
      }
  }
  __syncthreads();
  // row 34 = a ground-truth label above 33, column 34 = a predicted one
  for (int i = tid; i < kCells; i += 256)
    if (cnt[i] != 0 && (i / kL1 == kL || i % kL1 == kL))
      atomicOr(&flag[0], (i / kL1 == kL ? RA_PIXEL_STATUS_GT : 0) | (i % kL1 == kL ? RA_PIXEL_STATUS_PRED : 0));
  __syncthreads();
  int *rec = part + ((size_t)b * gridDim.x + blockIdx.x) * kRec;
  for (int i = tid; i < kCells; i += 256) rec[i] = cnt[i];
  rec[kItp + tid] = itp[tid];
  rec[kIctp + tid] = ictp[tid];
  if (tid == 0) rec[kFlag] = flag[0];
}

// Workgroup x < kConfJobs adds 16 cells of the table: per image the nwg partials, dealt over 16 slices (w = tid >> 4, + 16,
// ...) that meet in LDS — the image's int32 count — and the images one after the other into an int64 that is ADDED to conf.
// One thread owns a cell: no atomics.  The other workgroups, kInstJobs per image, add 16 of the image's 512 instance counters
// the same way; the first of them also gathers the image's status bits.
__global__ __launch_bounds__(256) void confusion_finish_kernel(const int *part, int nwg, int B, unsigned long long *conf,
                                                                int *inst_tp, int *inst_cat_tp, int *status) {
  __shared__ int red[256], flag[1];
  const int tid = threadIdx.x, col = tid & (kFinCols - 1), slice = tid / kFinCols;
  if ((int)blockIdx.x < kConfJobs) {
    const int e = blockIdx.x * kFinCols + col;
    long long tot = 0;
    for (int b = 0; b < B; ++b) {
      int a = 0;
      if (e < kCells) {
        const int *p = part + (size_t)b * nwg * kRec + e;
#pragma unroll 8
        for (int w = slice; w < nwg; w += 256 / kFinCols) a += p[(size_t)w * kRec];
      }
      red[tid] = a;
      __syncthreads();
      if (tid < kFinCols) {
        int s = 0;
        for (int k = 0; k < 256 / kFinCols; ++k) s += red[tid + k * kFinCols];
        tot += s;
      }
      __syncthreads();
    }
    if (tid < kFinCols && e < kCells) {
      const int gi = e / kL1, pi = e % kL1;
      if (gi < kL && pi < kL) conf[gi * kL + pi] += (unsigned long long)tot;
    }
    return;
  }
  const int job = blockIdx.x - kConfJobs, b = job / kInstJobs, chunk = job % kInstJobs;
  const int k = chunk * kFinCols + col;  // < 512: inst_tp then inst_cat_tp
  const int *p = part + (size_t)b * nwg * kRec + kItp + k;
  int a = 0;
#pragma unroll 8
  for (int w = slice; w < nwg; w += 256 / kFinCols) a += p[(size_t)w * kRec];
  red[tid] = a;
  if (tid == 0) flag[0] = 0;
  __syncthreads();
  if (tid < kFinCols) {
    int s = 0;
    for (int q = 0; q < 256 / kFinCols; ++q) s += red[tid + q * kFinCols];
    (k < kMaxGt ? inst_tp : inst_cat_tp)[(size_t)b * kMaxGt + (k & (kMaxGt - 1))] = s;
  }
  if (chunk != 0) return;  // uniform
  int f = 0;
  for (int w = tid; w < nwg; w += 256) f |= part[((size_t)b * nwg + w) * kRec + kFlag];
  if (f) atomicOr(&flag[0], f);
  __syncthreads();
  if (tid == 0) status[b] = flag[0];
}

inline bool plane_ok(int H, int W) { return H > 0 && W > 0 && (long long)H * W < (1ll << 31); }
inline int ntiles_of(long long HW) { return (int)((HW + kTile - 1) / kTile); }
inline int wgs_per_image(int B, long long HW) {
  const int tiles = ntiles_of(HW), want = kTargetWgs / B > 0 ? kTargetWgs / B : 1;
  return tiles < want ? tiles : want;
}
inline bool sem_ok(int Hs, int Ws, int C) { return plane_ok(Hs, Ws) && C >= kMinC && C <= kMaxC; }

int confusion(const char *who, const unsigned char *pred, const SemSrc *sem, const int *gt_ids, const unsigned char *gt_labels,
              const int *ids, const int *count, int B, int H, int W, int *ws, size_t ws_ints, unsigned long long *conf,
              int *inst_tp, int *inst_cat_tp, int *status, void *stream) {
  if ((!pred && !sem) || (sem && !sem->sem) || !gt_ids || !ids || !count || !ws || !conf || !inst_tp || !inst_cat_tp ||
      !status || B <= 0)
    return fail(RA_E_INVALID, "%s: bad argument", who);
  if (!plane_ok(H, W) || B > 65535 || (sem && !sem_ok(sem->Hs, sem->Ws, sem->C)))
    return fail(RA_E_SHAPE, "%s: %dx%d, B=%d, sem %dx%dx%d (H * W < 2^31, B <= 65535, %d <= C <= %d)", who, H, W, B,
                sem ? sem->Hs : 0, sem ? sem->Ws : 0, sem ? sem->C : 0, kMinC, kMaxC);
  if (ws_ints < ra_pixel_confusion_workspace_ints(B, H, W)) return fail(RA_E_WORKSPACE, "%s: workspace", who);
  const long long HW = (long long)H * W;
  const int nwg = wgs_per_image(B, HW), ntiles = ntiles_of(HW);
  const bool vec = HW % 4 == 0 && (reinterpret_cast<uintptr_t>(gt_ids) & 15) == 0 &&
                   (reinterpret_cast<uintptr_t>(gt_labels) & 3) == 0 && (reinterpret_cast<uintptr_t>(pred) & 3) == 0;
  hipStream_t st = as_stream(stream);
  const dim3 grid(nwg, B), block(256);
  const SemSrc s = sem ? *sem : SemSrc{nullptr, 0, 0, 0, 0.0, 0.0};
#define RA_PIX_LAUNCH(SEM, VEC) \
  hipLaunchKernelGGL((confusion_kernel<SEM, VEC>), grid, block, 0, st, pred, s, gt_ids, gt_labels, ids, count, (unsigned)HW, W, ntiles, ws)
  if (sem) {
    if (vec) RA_PIX_LAUNCH(true, true);
    else RA_PIX_LAUNCH(true, false);
  } else {
    if (vec) RA_PIX_LAUNCH(false, true);
    else RA_PIX_LAUNCH(false, false);
  }
#undef RA_PIX_LAUNCH
  if (int rc = launch_status(who)) return rc;
  hipLaunchKernelGGL(confusion_finish_kernel, dim3(kConfJobs + B * kInstJobs), block, 0, st, ws, nwg, B, conf, inst_tp,
                     inst_cat_tp, status);
  return launch_status(who);
}

}  // namespace pix
}  // namespace ra

using namespace ra;

extern "C" int ra_sem_labels_u8(const float *sem, int B, int Hs, int Ws, int C, int H, int W, unsigned char *labels,
                                void *stream) {
  if (!sem || !labels || B <= 0) return fail(RA_E_INVALID, "ra_sem_labels_u8: bad argument");
  if (!pix::sem_ok(Hs, Ws, C) || !pix::plane_ok(H, W) || B > 65535)
    return fail(RA_E_SHAPE, "ra_sem_labels_u8: sem %dx%dx%d -> %dx%d, B=%d (%d <= C <= %d, planes below 2^31 pixels, B <= 65535)",
                Hs, Ws, C, H, W, B, pix::kMinC, pix::kMaxC);
  const long long HW = (long long)H * W;
  const pix::SemSrc s{sem, Hs, Ws, C, (double)Hs / (double)H, (double)Ws / (double)W};
  hipLaunchKernelGGL(pix::sem_labels_kernel, dim3((unsigned)((HW + 255) / 256), B), dim3(256), 0, as_stream(stream), s,
                     (unsigned)HW, W, labels);
  return launch_status("ra_sem_labels_u8");
}

extern "C" size_t ra_pixel_confusion_workspace_ints(int B, int H, int W) {
  if (B <= 0 || !pix::plane_ok(H, W)) return 0;
  return (size_t)B * pix::wgs_per_image(B, (long long)H * W) * pix::kRec;
}

extern "C" int ra_pixel_confusion_u8(const unsigned char *pred, const int *gt_ids, const unsigned char *gt_labels,
                                     const int *ids, const int *count, int B, int H, int W, int *ws, size_t ws_ints,
                                     unsigned long long *conf, int *inst_tp, int *inst_cat_tp, int *status, void *stream) {
  if (!pred) return fail(RA_E_INVALID, "ra_pixel_confusion_u8: bad argument");
  return pix::confusion("ra_pixel_confusion_u8", pred, nullptr, gt_ids, gt_labels, ids, count, B, H, W, ws, ws_ints, conf,
                        inst_tp, inst_cat_tp, status, stream);
}

extern "C" int ra_pixel_confusion_sem_f32(const float *sem, int Hs, int Ws, int C, const int *gt_ids,
                                          const unsigned char *gt_labels, const int *ids, const int *count, int B, int H,
                                          int W, int *ws, size_t ws_ints, unsigned long long *conf, int *inst_tp,
                                          int *inst_cat_tp, int *status, void *stream) {
  if (!sem) return fail(RA_E_INVALID, "ra_pixel_confusion_sem_f32: bad argument");
  const pix::SemSrc s{sem, Hs, Ws, C, H > 0 ? (double)Hs / (double)H : 0.0, W > 0 ? (double)Ws / (double)W : 0.0};
  return pix::confusion("ra_pixel_confusion_sem_f32", nullptr, &s, gt_ids, gt_labels, ids, count, B, H, W, ws, ws_ints, conf,
                        inst_tp, inst_cat_tp, status, stream);
}
