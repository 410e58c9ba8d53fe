// K15 — the matching step of the Cityscapes instance-level evaluation (evalInstanceLevelSemanticLabeling.py:260-353,
// assignGt2Preds; instances2dict.py:37-40), behind the output stage K14 while the masks are still on the device.
//
//   catalogue   np.unique(gt, return_counts=True) of one image of *_gtFine_instanceIds.png values: the distinct ids in
//               ascending order and their pixel counts.  Two launches.  cat_partial: every workgroup walks tiles of one image
//               and keeps what it meets in a 512-entry hash table in LDS; cat_merge: one workgroup per image adds the
//               workgroups' tables in a table of its own, ranks the keys and writes the sorted catalogue.  No global
//               atomics and no table indexed by an id: an id outside [0, 65535] or beyond the cap goes to a reject counter
//               and raises the image's status word.
//               cat_partial is a template over the geometry source of ra_ragged.h: a batch of mixed full sizes in one flat
//               buffer takes the same two launches (ra_gt_instance_catalog_ragged_i32).
//   overlap     inter[b,t,g] = count_nonzero(gt == id_g & y[b,t] != 0) (:333) and pred_pixels[b,t] = count_nonzero(y[b,t]
//               != 0) (:306-307) — a joint histogram.  A workgroup walks tiles of 1024 pixels of one image: 16 bytes of
//               gt_ids per lane, the slot of each id by a binary search in the catalogue (LDS), then y plane by plane, 16
//               bytes per lane, each byte of y and gt_ids read once.  The counters [T][256] live in LDS.  A wave covers 256
//               consecutive pixels, which mostly lie on ONE catalogue entry: then the wave's count of a plane is four
//               ballots and four population counts in scalar registers and ONE LDS add, however many of its lanes the mask
//               covers.  Only a wave that straddles entries adds per lane (per run of equal slots among its 4 pixels).
//               Every workgroup leaves its counters in ws and a finishing launch adds them: integers, so the result is
//               exact and the same from run to run.
//
// kMaxGt = 256 distinct ids per image is a constant of these kernels (LDS counters: T x 256 ints = 32 KB at T = 32).  It
// rests on NO measurement of the real dataset made here: the dataset is not available to this project.  An image with
// more gets status bit RA_GT_STATUS_COUNT, which the caller turns into an error naming the image.
#include <cstdint>

#include "ra_common.h"
#include "ra_gt_ids.h"
#include "ra_ragged.h"

namespace ra {
namespace iov {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
constexpr int kMaxT = 32;                // the evaluator's limit (ra_eval.hip)
constexpr int kMaxGt = RA_OVERLAP_MAX_GT;  // 256, see above
constexpr int kMaxId = 65535;            // the 16-bit PNG
constexpr int kTile = 1024;              // pixels per tile: 256 threads x 4
constexpr int kHash = 512;               // entries of a workgroup's table (twice the cap, so probes stay short)
constexpr int kCatWgs = 256;             // catalogue: workgroups in all (an image of 8 MB: 8 tiles each)
constexpr int kTargetWgs = 1024;         // overlap: four workgroups per CU
constexpr int kKU = 5;                   // planes of y in flight per lane (T = 20: four rounds)
constexpr int kFinCols = 16;             // finishing launch: columns of inter per workgroup; 256 / 16 slices of the partials
constexpr int kPartStride = 2 * kHash + 4;  // ints of one workgroup's record: n, flags, reject, pad, keys[512], counts[512]

// this lane's 4 consecutive ints / floats at `base` of a plane of HW elements; beyond the plane: fill
__device__ __forceinline__ i32x4 load_ids(const int *p, unsigned base, unsigned HW, int vec_ok) {
  i32x4 v = {-1, -1, -1, -1};
  if (vec_ok) {  // HW % 4 == 0 and 16-byte aligned: base < HW implies base + 3 < HW
    if (base < HW) v = *reinterpret_cast<const i32x4 *>(p + base);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (base + j < HW) v[j] = p[base + j];
  }
  return v;
}

// (key, c) into an open-addressing table of kHash entries (keys -1 = free).  A key outside [0, kMaxId] or a full table goes
// to rej[0] and raises flags[0]; nothing is indexed by the key itself.
__device__ __forceinline__ void hash_add(int *keys, int *cnts, int *rej, int *flags, int key, int c) {
  if (key < 0 || key > kMaxId) {
    atomicAdd(rej, c);
    atomicOr(flags, RA_GT_STATUS_RANGE);
    return;
  }
  unsigned h = ((unsigned)key * 2654435761u) >> 23;  // 9 bits
  for (int probe = 0; probe < kHash; ++probe) {
    const int old = atomicCAS(&keys[h], -1, key);
    if (old == -1 || old == key) {
      atomicAdd(&cnts[h], c);
      return;
    }
    h = (h + 1) & (kHash - 1);
  }
  atomicAdd(rej, c);
  atomicOr(flags, RA_GT_STATUS_COUNT);
}

// Workgroup (x, b) walks the tiles x, x + gridDim.x, ... of image b.  Per tile a wave peels the distinct ids of its 256 pixels
// (one iteration each: the id of the first lane that still has one, four ballots, four population counts) and carries the
// last id and its count in scalar registers from tile to tile, so a run of equal ids costs one table update when it ends.
// GEO: geo::Uniform (gt [B,h,w]) or geo::Ragged (gt flat, image b at its table entry).  A workgroup whose image has fewer tiles
// than the grid is wide walks none and leaves an empty record.
template <class GEO>
__global__ __launch_bounds__(256) void cat_partial_kernel(const int *gt, const GEO src, int *part) {
  __shared__ int keys[kHash], cnts[kHash], misc[4];  // misc: n, flags, reject
  const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
  for (int i = tid; i < kHash; i += 256) keys[i] = -1, cnts[i] = 0;
  if (tid < 4) misc[tid] = 0;
  __syncthreads();
  const geo::Image im = src.at(b);
  const unsigned HW = (unsigned)im.h * (unsigned)im.w;  // < 2^31
  const int ntiles = (int)((HW + kTile - 1) / kTile), vec_ok = im.vec;
  const int *g = gt + im.off;
  int run_key = -1, run_cnt = 0;  // wave-uniform
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const unsigned base = (unsigned)tile * kTile + 4 * tid;  // < 2^31 + kTile
    const i32x4 v = load_ids(g, base, HW, vec_ok);
    bool ok[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) ok[j] = base + j < HW;  // still to be counted
    for (;;) {
      const bool mine = ok[0] || ok[1] || ok[2] || ok[3];
      const unsigned long long left = __ballot(mine);
      if (!left) break;
      const int src = __ffsll((long long)left) - 1;
      const int cand = ok[0] ? v[0] : ok[1] ? v[1] : ok[2] ? v[2] : v[3];
      const int k = __shfl(cand, src, 64);  // uniform
      int tot = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool hit = ok[j] && v[j] == k;
        tot += __popcll(__ballot(hit));
        ok[j] = ok[j] && !hit;
      }
      if (k != run_key) {
        if (run_cnt && lane == 0) hash_add(keys, cnts, &misc[2], &misc[1], run_key, run_cnt);
        run_key = k, run_cnt = 0;
      }
      run_cnt += tot;
    }
  }
  if (run_cnt && lane == 0) hash_add(keys, cnts, &misc[2], &misc[1], run_key, run_cnt);
  __syncthreads();
  int *rec = part + ((size_t)b * gridDim.x + blockIdx.x) * kPartStride;
  for (int i = tid; i < kHash; i += 256)
    if (keys[i] >= 0) {
      const int pos = atomicAdd(&misc[0], 1);  // < kHash
      rec[4 + pos] = keys[i];
      rec[4 + kHash + pos] = cnts[i];
    }
  __syncthreads();
  if (tid < 3) rec[tid] = misc[tid];
}

// One workgroup per image: thread w adds the records of the workgroups w, w + 256, ... into one table, every key is ranked
// among the keys (the table is small: 512 x 512 comparisons), and the first kMaxGt in ascending order are written.
__global__ __launch_bounds__(256) void cat_merge_kernel(const int *part, int nwg, int *ids, int *pixels, int *count,
                                                         int *status) {
  __shared__ int keys[kHash], cnts[kHash], misc[4];  // misc: n, flags, reject
  const int b = blockIdx.x, tid = threadIdx.x;
  for (int i = tid; i < kHash; i += 256) keys[i] = -1, cnts[i] = 0;
  if (tid < 4) misc[tid] = 0;
  __syncthreads();
  for (int w = tid; w < nwg; w += 256) {
    const int *rec = part + ((size_t)b * nwg + w) * kPartStride;
    int n = rec[0];
    n = n < 0 ? 0 : (n > kHash ? kHash : n);
    if (rec[1]) atomicOr(&misc[1], rec[1]);
    if (rec[2]) atomicAdd(&misc[2], rec[2]);
    for (int i = 0; i < n; ++i) hash_add(keys, cnts, &misc[2], &misc[1], rec[4 + i], rec[4 + kHash + i]);
  }
  __syncthreads();
  int *oid = ids + (size_t)b * kMaxGt, *opx = pixels + (size_t)b * kMaxGt;
  for (int i = tid; i < kHash; i += 256) {
    const int k = keys[i];
    if (k < 0) continue;
    int rank = 0;
    for (int j = 0; j < kHash; ++j) rank += (keys[j] >= 0 && keys[j] < k) ? 1 : 0;
    atomicAdd(&misc[0], 1);
    if (rank < kMaxGt) oid[rank] = k, opx[rank] = cnts[i];
  }
  __syncthreads();
  const int n = misc[0];
  for (int i = tid; i < kMaxGt; i += 256)
    if (i >= n) oid[i] = -1, opx[i] = 0;
  if (tid == 0) {
    count[b] = n < kMaxGt ? n : kMaxGt;
    status[b] = misc[1] | (n > kMaxGt ? RA_GT_STATUS_COUNT : 0);
  }
}

using gtid::find_slot;  // the slot of an id in the sorted catalogue, -1 when it is not there

// Workgroup (x, b) walks the tiles x, x + gridDim.x, ... of image b; see the head of the file.  sh: cnt[T][256], pp[32],
// cat[256].  VEC: 16-byte loads (H * W % 4 == 0, y and gt_ids 16-byte aligned), else element loads.  Its counters go to
// parts[b][x][t][g < n] and partp[b][x][t].
template <bool VEC>
__global__ __launch_bounds__(256) void overlap_kernel(const float *y, const int *gt, const int *ids, const int *count, int T,
                                                       unsigned HW, int ntiles, int *parts, int *partp) {
  extern __shared__ __attribute__((aligned(16))) int sh[];
  int *cnt = sh, *pp = sh + T * kMaxGt, *cat = pp + kMaxT;
  const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
  int n = count[b];
  n = n < 0 ? 0 : (n > kMaxGt ? kMaxGt : n);
  for (int i = tid; i < T * kMaxGt; i += 256) cnt[i] = 0;
  if (tid < kMaxT) pp[tid] = 0;
  cat[tid] = tid < n ? ids[(size_t)b * kMaxGt + tid] : 0x7fffffff;
  __syncthreads();
  const int *g = gt + (size_t)b * HW;
  const float *yb = y + (size_t)b * T * HW;

  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const unsigned base = (unsigned)tile * kTile + 4 * tid;  // < 2^31 + kTile
    const i32x4 id = load_ids(g, base, HW, VEC);
    int s[4];
    s[0] = find_slot(cat, n, id[0]);
#pragma unroll
    for (int j = 1; j < 4; ++j) s[j] = id[j] == id[j - 1] ? s[j - 1] : find_slot(cat, n, id[j]);
    const int u = __builtin_amdgcn_readfirstlane(s[0]);
    const bool uni = __all(s[0] == u && s[1] == u && s[2] == u && s[3] == u);  // the whole wave on one entry
    for (int t0 = 0; t0 < T; t0 += kKU) {
      f32x4 v[kKU];
#pragma unroll
      for (int k = 0; k < kKU; ++k) {
        v[k] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (t0 + k < T) {
          const float *q = yb + (size_t)(t0 + k) * HW + base;
          if (VEC) {
            if (base < HW) v[k] = __builtin_nontemporal_load(reinterpret_cast<const f32x4 *>(q));
          } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
              if (base + j < HW) v[k][j] = q[j];
          }
        }
      }
#pragma unroll
      for (int k = 0; k < kKU; ++k) {
        const int t = t0 + k;
        if (t >= T) break;
        int tot = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) tot += __popcll(__ballot(v[k][j] != 0.f));  // :306; a NaN counts, as in numpy
        if (tot == 0) continue;  // uniform
        if (lane == 0) atomicAdd(&pp[t], tot);
        if (uni) {
          if (u >= 0 && lane == 0) atomicAdd(&cnt[t * kMaxGt + u], tot);
        } else {
          int c = 0;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            c += v[k][j] != 0.f ? 1 : 0;
            if (j == 3 || s[j + 1] != s[j]) {  // the end of a run of equal slots
              if (c && s[j] >= 0) atomicAdd(&cnt[t * kMaxGt + s[j]], c);
              c = 0;
            }
          }
        }
      }
    }
  }
  __syncthreads();
  const size_t wg = (size_t)b * gridDim.x + blockIdx.x;
  int *ps = parts + wg * T * kMaxGt;
  for (int i = tid; i < T * kMaxGt; i += 256)
    if ((i & (kMaxGt - 1)) < n) ps[i] = cnt[i];
  if (tid < T) partp[wg * T + tid] = pp[tid];
}

// Workgroup (t, b, cb) adds the nwg partials of the 16 columns g = 16 cb + (tid & 15) of inter[b,t,:]: the partials are
// dealt over 16 slices (w = tid >> 4, + 16, ...), eight loads in flight per thread, and the slices meet in LDS; integers, so
// the order does not matter.  Column blocks beyond the image's n entries write their zeros and leave.  (One thread per column
// walking all nwg partials one load after the other, 20 workgroups in all at B = 1, took 157 us of the 246 us of both ops.)
// The workgroups cb = 0 also add the partials of pred_pixels[b,t].
__global__ __launch_bounds__(256) void overlap_finish_kernel(const int *parts, const int *partp, const int *count, int nwg,
                                                              int T, int *inter, int *pred_pixels) {
  __shared__ int red[256];
  const int t = blockIdx.x, b = blockIdx.y, cb = blockIdx.z, tid = threadIdx.x;
  int n = count[b];
  n = n < 0 ? 0 : (n > kMaxGt ? kMaxGt : n);
  const int g = cb * kFinCols + (tid & (kFinCols - 1));  // < kMaxGt
  int *out = inter + ((size_t)b * T + t) * kMaxGt;
  if (cb * kFinCols >= n) {  // uniform
    if (tid < kFinCols) out[g] = 0;
  } else {
    int a = 0;
    if (g < n) {  // the overlap kernel wrote columns < n only
      const int *p = parts + ((size_t)b * nwg * T + t) * kMaxGt + g;
#pragma unroll 8
      for (int w = tid / kFinCols; w < nwg; w += 256 / kFinCols) a += p[(size_t)w * T * kMaxGt];
    }
    red[tid] = a;
    __syncthreads();
    for (int off = 128; off >= kFinCols; off >>= 1) {
      if (tid < off) red[tid] += red[tid + off];
      __syncthreads();
    }
    if (tid < kFinCols) out[g] = red[tid];
  }
  if (cb != 0) return;  // uniform
  __syncthreads();
  int q = 0;
  for (int w = tid; w < nwg; w += 256) q += partp[((size_t)b * nwg + w) * T + t];
  red[tid] = q;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (tid < off) red[tid] += red[tid + off];
    __syncthreads();
  }
  if (tid == 0) pred_pixels[(size_t)b * T + t] = red[0];
}

inline bool plane_ok(int H, int W) { return H > 0 && W > 0 && (long long)H * W < (1ll << 31); }
inline int ntiles_of(long long HW) { return (int)((HW + kTile - 1) / kTile); }
inline int cat_wgs(int B, long long HW) {
  const int tiles = ntiles_of(HW), want = kCatWgs / B > 0 ? kCatWgs / B : 1;
  return tiles < want ? tiles : want;
}
inline int ov_wgs(int B, long long HW) {
  const int tiles = ntiles_of(HW), want = kTargetWgs / B > 0 ? kTargetWgs / B : 1;
  return tiles < want ? tiles : want;
}

}  // namespace iov
}  // namespace ra

using namespace ra;

extern "C" size_t ra_gt_instance_catalog_workspace_ints(int B, int H, int W) {
  if (B <= 0 || !iov::plane_ok(H, W)) return 0;
  return (size_t)B * iov::cat_wgs(B, (long long)H * W) * iov::kPartStride;
}

extern "C" int ra_gt_instance_catalog_i32(const int *gt_ids, int B, int H, int W, int *ws, size_t ws_ints, int *ids,
                                          int *pixels, int *count, int *status, void *stream) {
  if (!gt_ids || !ws || !ids || !pixels || !count || !status || B <= 0)
    return fail(RA_E_INVALID, "ra_gt_instance_catalog_i32: bad argument");
  if (!iov::plane_ok(H, W) || B > 65535)
    return fail(RA_E_SHAPE, "ra_gt_instance_catalog_i32: gt_ids %dx%d, B=%d (H * W < 2^31, B <= 65535)", H, W, B);
  if (ws_ints < ra_gt_instance_catalog_workspace_ints(B, H, W))
    return fail(RA_E_WORKSPACE, "ra_gt_instance_catalog_i32: workspace");
  const long long HW = (long long)H * W;
  const int nwg = iov::cat_wgs(B, HW);
  const int vec_ok = HW % 4 == 0 && (reinterpret_cast<uintptr_t>(gt_ids) & 15) == 0;
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(iov::cat_partial_kernel<geo::Uniform>, dim3(nwg, B), dim3(256), 0, st, gt_ids, geo::Uniform{H, W, vec_ok}, ws);
  if (int rc = launch_status("ra_gt_instance_catalog_i32")) return rc;
  hipLaunchKernelGGL(iov::cat_merge_kernel, dim3(B), dim3(256), 0, st, ws, nwg, ids, pixels, count, status);
  return launch_status("ra_gt_instance_catalog_i32 (merge)");
}

extern "C" size_t ra_gt_instance_catalog_ragged_workspace_ints(const ra_image_geo *geo, int B) {
  const long long px = geo::max_pixels(geo, B);
  if (B <= 0 || px <= 0 || px >= (1ll << 31)) return 0;
  return (size_t)B * iov::cat_wgs(B, px) * iov::kPartStride;
}

extern "C" int ra_gt_instance_catalog_ragged_i32(const int *gt_ids, size_t total, const ra_image_geo *geo, ra_image_geo *geo_dev,
                                                 int B, int *ws, size_t ws_ints, int *ids, int *pixels, int *count, int *status,
                                                 void *stream) {
  const char *who = "ra_gt_instance_catalog_ragged_i32";
  if (!gt_ids || !geo || !geo_dev || !ws || !ids || !pixels || !count || !status || B <= 0)
    return fail(RA_E_INVALID, "%s: bad argument", who);
  if (B > 65535) return fail(RA_E_SHAPE, "%s: B=%d (B <= 65535)", who, B);
  if (int rc = geo::check(who, geo, B, total, (1ll << 31) - 1, "h * w < 2^31")) return rc;
  if (ws_ints < ra_gt_instance_catalog_ragged_workspace_ints(geo, B)) return fail(RA_E_WORKSPACE, "%s: workspace", who);
  const int nwg = iov::cat_wgs(B, geo::max_pixels(geo, B));  // the largest image's tiles; an image's own count bounds its walk
  const int vec = (reinterpret_cast<uintptr_t>(gt_ids) & 15) == 0;
  hipStream_t st = as_stream(stream);
  if (int rc = geo::upload(who, geo, geo_dev, B, st)) return rc;
  hipLaunchKernelGGL(iov::cat_partial_kernel<geo::Ragged>, dim3(nwg, B), dim3(256), 0, st, gt_ids, geo::Ragged{geo_dev, vec}, ws);
  if (int rc = launch_status(who)) return rc;
  hipLaunchKernelGGL(iov::cat_merge_kernel, dim3(B), dim3(256), 0, st, ws, nwg, ids, pixels, count, status);
  return launch_status("ra_gt_instance_catalog_ragged_i32 (merge)");
}

extern "C" size_t ra_instance_overlap_workspace_ints(int B, int T, int H, int W) {
  if (B <= 0 || T <= 0 || !iov::plane_ok(H, W)) return 0;
  return (size_t)B * iov::ov_wgs(B, (long long)H * W) * T * (iov::kMaxGt + 1);
}

extern "C" int ra_instance_overlap_f32(const float *y, const int *gt_ids, const int *ids, const int *count, int B, int T,
                                       int H, int W, int *ws, size_t ws_ints, int *inter, int *pred_pixels, void *stream) {
  if (!y || !gt_ids || !ids || !count || !ws || !inter || !pred_pixels || B <= 0)
    return fail(RA_E_INVALID, "ra_instance_overlap_f32: bad argument");
  if (T < 1 || T > iov::kMaxT || !iov::plane_ok(H, W) || B > 65535)
    return fail(RA_E_SHAPE, "ra_instance_overlap_f32: T=%d y %dx%d B=%d (1 <= T <= %d, H * W < 2^31, B <= 65535)", T, H, W, B,
                iov::kMaxT);
  if (ws_ints < ra_instance_overlap_workspace_ints(B, T, H, W))
    return fail(RA_E_WORKSPACE, "ra_instance_overlap_f32: workspace");
  const long long HW = (long long)H * W;
  const int nwg = iov::ov_wgs(B, HW);
  const int vec_ok = HW % 4 == 0 && ((reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(gt_ids)) & 15) == 0;
  int *parts = ws, *partp = ws + (size_t)B * nwg * T * iov::kMaxGt;
  const size_t lds = (size_t)(T * iov::kMaxGt + iov::kMaxT + iov::kMaxGt) * sizeof(int);
  hipStream_t st = as_stream(stream);
  if (vec_ok)
    hipLaunchKernelGGL(iov::overlap_kernel<true>, dim3(nwg, B), dim3(256), lds, st, y, gt_ids, ids, count, T, (unsigned)HW,
                       iov::ntiles_of(HW), parts, partp);
  else
    hipLaunchKernelGGL(iov::overlap_kernel<false>, dim3(nwg, B), dim3(256), lds, st, y, gt_ids, ids, count, T, (unsigned)HW,
                       iov::ntiles_of(HW), parts, partp);
  if (int rc = launch_status("ra_instance_overlap_f32")) return rc;
  hipLaunchKernelGGL(iov::overlap_finish_kernel, dim3(T, B, iov::kMaxGt / iov::kFinCols), dim3(256), 0, st, parts, partp, count, nwg, T, inter, pred_pixels);
  return launch_status("ra_instance_overlap_f32 (finish)");
}
