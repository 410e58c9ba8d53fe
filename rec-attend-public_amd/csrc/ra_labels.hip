// K17 — the label stage in front of training and of the pre-stage's evaluation: y_gt, s_gt, d_gt, c_gt and the full-size
// foreground from instance-id images (setup_cityscapes.py / setup_kitti.py / setup_cvppp.py: data_api/ins_seg_assembler.py:
// 85-155, data_api/sep_labels.py, data_api/orientation.py:31-85, read back by data_api/ins_seg_dataset.py:158-172,216-236,
// 257-271).  The reference cuts one full-size mask per id, resizes each with cv2.resize(..., INTER_NEAREST) and stacks them;
// here the id image is sampled at the network pixels and ids are compared, which is the same thing: no full-size
// per-instance mask exists.  The instances of an image are the entries of its catalogue (ra_gt_instance_catalog_i32,
// np.unique of the FULL image as sep_labels takes it: an instance that vanishes at network size still counts) that the
// dataset rule accepts.
//
//   moments   one pass over the H x W SAMPLED positions: id -> catalogue slot (binary search in LDS), per slot area, sum of
//             rows, sum of columns in 64-bit integer counters in LDS.  A wave whose 64 pixels lie on one slot adds once.
//             Every workgroup leaves its counters of the slots < count in ws.
//   rank      one workgroup per image, thread g = slot g: adds the workgroups' counters in a fixed order, applies the
//             dataset rule, ranks the accepted slots by area descending (ties: the larger slot first) and writes num_obj,
//             s_gt, inst_id, area, sem_cls, and for the fill the table slot -> (rank, class) and the centroids
//             sum / (area + 1e-7) in double.
//   fill      one thread per 4 consecutive network pixels: id -> slot -> rank, then ALL T planes of y_gt for those pixels
//             (zeros included: no memset, no scatter), d_cls, d_gt, c_gt; 16-byte stores when H * W % 4 == 0 and the
//             outputs are 16-byte aligned, element stores otherwise.  The orientation class is evaluated in double in
//             the reference's order (orientation.py:58-73), built without contraction to fused multiply-adds.
//   fg_full   fg_model_eval.py:142-143: 1 where the dataset rule accepts the id, over the full-size image, 16 bytes of ids
//             per lane where aligned.  The rule is applied to the id itself: for an image whose catalogue status is 0 that is
//             the set of accepted catalogue entries.
//
// Integer counters and a fixed order of addition: exact, and the same bits on every run.  Nothing is indexed by an id.
// Mixed full sizes in one batch (ra_labels_assemble_ragged_i32): moments, fill and fg_full are templates over the geometry source of
// ra_ragged.h; the network-size outputs stay dense, the sampling scales become each image's own, fg_full is written flat.
#include <cmath>
#include <cstdint>

#include "ra_common.h"
#include "ra_gt_ids.h"
#include "ra_ragged.h"

namespace ra {
namespace lab {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef unsigned long long u64;
constexpr int kMaxT = RA_LABELS_MAX_T;
constexpr int kMaxGt = RA_OVERLAP_MAX_GT;  // 256 = threads per workgroup: thread g owns slot g in rank_kernel
constexpr int kMaxId = 65535;              // the 16-bit PNG, as the catalogue has it
constexpr int kMomWgs = 512;               // moments: workgroups in all (two per CU)
constexpr int kFillPix = 1024;             // fill, fg_full: pixels per workgroup (256 threads x 4)
static_assert(kMaxGt == 256, "rank_kernel: one thread per catalogue slot");

// the dataset rule (data_api/cvppp.py:49-63, kitti.py:51-65; cityscapes.py:106-118): is `id` an instance, and of which class
__device__ __forceinline__ bool accept(int dataset, int id, int &cls) {
  cls = -1;
  if (id <= 0 || id > kMaxId) return false;  // 0 is the background everywhere; beyond: not in any catalogue
  if (dataset == RA_LABELS_PLAIN) {
    cls = 0;
    return true;
  }
  if (id <= 1000) return false;
  cls = gtid::cs_class_of(id / 1000);
  return cls >= 0;
}

// cv2.resize(..., INTER_NEAREST): destination index d reads source index min(floor(d * scale), n_src - 1), scale =
// 1.0 / ((double)n_dst / n_src) in double (OpenCV's resizeNN: ifx = 1. / inv_scale_x)
__device__ __forceinline__ int nn_src(int d, double scale, int n_src) {
  const int s = (int)floor((double)d * scale);
  return s < n_src - 1 ? s : n_src - 1;
}

__device__ __forceinline__ int clamp_count(int n) { return n < 0 ? 0 : (n > kMaxGt ? kMaxGt : n); }

// The sampling of image b: where its ids start, its full size and the scales of nn_src.  GEO = geo::Uniform: gt is [B,Hf,Wf] and
// the scales are the launch's (formed on the host); geo::Ragged: gt is flat, the image's table entry gives offset and size, and
// the scales are the same double expressions 1.0 / ((double)H / Hf), evaluated once per workgroup (IEEE division: the same bits).
struct Sampling {
  const int *g;
  int Hf, Wf;
  double sy, sx;
};
template <class GEO>
__device__ __forceinline__ Sampling sampling_of(const int *gt, const GEO &src, int b, int H, int W, double sy, double sx) {
  const geo::Image im = src.at(b);
  if (GEO::kRagged) {
    sy = 1.0 / ((double)H / (double)im.h);
    sx = 1.0 / ((double)W / (double)im.w);
  }
  return Sampling{gt + im.off, im.h, im.w, sy, sx};
}

// Workgroup (x, b) walks the tiles (256 network pixels) x, x + gridDim.x, ... of image b.
// part[b][x][q][g < n], q = area, sum of rows, sum of columns.
template <class GEO>
__global__ __launch_bounds__(256) void moments_kernel(const int *gt, const int *ids, const int *count, const GEO src, int H, int HW,
                                                       int W, double sy_, double sx_, int ntiles, u64 *part) {
  __shared__ int cat[kMaxGt];
  __shared__ u64 m[3][kMaxGt];
  const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
  const int n = clamp_count(count[b]);
  cat[tid] = tid < n ? ids[(size_t)b * kMaxGt + tid] : 0x7fffffff;
  m[0][tid] = m[1][tid] = m[2][tid] = 0;
  __syncthreads();
  const Sampling sm = sampling_of(gt, src, b, H, W, sy_, sx_);
  const int *g = sm.g;
  const int Hf = sm.Hf, Wf = sm.Wf;
  const double sy = sm.sy, sx = sm.sx;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const unsigned p = (unsigned)tile * 256 + tid;  // < 2^31 + 256
    int s = -1, r = 0, c = 0;
    if (p < (unsigned)HW) {
      r = (int)(p / (unsigned)W), c = (int)(p - (unsigned)r * W);
      s = gtid::find_slot(cat, n, g[(size_t)nn_src(r, sy, Hf) * Wf + nn_src(c, sx, Wf)]);
    }
    const int u = __builtin_amdgcn_readfirstlane(s);
    if (__all(s == u)) {  // the whole wave on one slot (or on none)
      if (u >= 0) {
        long long sr = r, sc = c;
        for (int off = 32; off > 0; off >>= 1) sr += __shfl_xor(sr, off, 64), sc += __shfl_xor(sc, off, 64);
        if (lane == 0) {
          atomicAdd(&m[0][u], (u64)64);
          atomicAdd(&m[1][u], (u64)sr);
          atomicAdd(&m[2][u], (u64)sc);
        }
      }
    } else if (s >= 0) {
      atomicAdd(&m[0][s], (u64)1);
      atomicAdd(&m[1][s], (u64)r);
      atomicAdd(&m[2][s], (u64)c);
    }
  }
  __syncthreads();
  u64 *ps = part + ((size_t)b * gridDim.x + blockIdx.x) * 3 * kMaxGt;
  if (tid < n) {
#pragma unroll
    for (int q = 0; q < 3; ++q) ps[q * kMaxGt + tid] = m[q][tid];
  }
}

// One workgroup per image; thread g owns catalogue slot g.  tab[b][g] = rank | class << 16 of an accepted slot, -1 else;
// cen[b][0][g], cen[b][1][g] = the centroid's row and column.
__global__ __launch_bounds__(256) void rank_kernel(const u64 *part, int nwg, const int *ids, const int *count, int T,
                                                    int dataset, int *num_obj, float *s_gt, int *inst_id, int *area,
                                                    int *sem_cls, int *tab, double *cen) {
  __shared__ int sh_area[kMaxGt];
  const int b = blockIdx.x, g = threadIdx.x;
  const int n = clamp_count(count[b]);
  u64 a = 0, sr = 0, sc = 0;
  if (g < n) {
    const u64 *p = part + (size_t)b * nwg * 3 * kMaxGt + g;
#pragma unroll 4
    for (int w = 0; w < nwg; ++w) {
      a += p[0], sr += p[kMaxGt], sc += p[2 * kMaxGt];
      p += 3 * kMaxGt;
    }
  }
  const int id = g < n ? ids[(size_t)b * kMaxGt + g] : -1;
  int cls;
  const bool acc = accept(dataset, id, cls);
  const int ar = (int)a;  // <= H * W < 2^31
  sh_area[g] = acc ? ar : -1;
  const int nobj = __syncthreads_count(acc);
  // ins_seg_dataset.py:169-172, np.argsort(area)[::-1]: descending, equal areas in descending catalogue order (a stable
  // ascending sort read backwards)
  int rank = 0;
  if (acc)
    for (int j = 0; j < n; ++j) {
      const int aj = sh_area[j];
      rank += (aj > ar || (aj == ar && j > g)) ? 1 : 0;
    }
  tab[(size_t)b * kMaxGt + g] = acc ? (rank | cls << 16) : -1;
  const double den = (double)a + 1e-7;  // orientation.py:51-53
  cen[((size_t)b * 2 + 0) * kMaxGt + g] = (double)sr / den;
  cen[((size_t)b * 2 + 1) * kMaxGt + g] = (double)sc / den;
  if (g == 0 && num_obj) num_obj[b] = nobj;
  if (g < T) {  // the slots no instance fills; the others are written by their instance below (ranks are distinct)
    if (s_gt) s_gt[(size_t)b * T + g] = g < nobj ? 1.f : 0.f;  // ins_seg_dataset.py:267-271
    if (g >= nobj) {
      if (inst_id) inst_id[(size_t)b * T + g] = -1;
      if (area) area[(size_t)b * T + g] = 0;
      if (sem_cls) sem_cls[(size_t)b * T + g] = -1;
    }
  }
  if (acc && rank < T) {
    if (inst_id) inst_id[(size_t)b * T + rank] = id;
    if (area) area[(size_t)b * T + rank] = ar;
    if (sem_cls) sem_cls[(size_t)b * T + rank] = cls;
  }
}

// orientation.py:58-73 for the pixel (r, c) of an instance with centroid (cy, cx), in double and in the reference's order
__device__ __forceinline__ int orientation_class(int r, int c, double cy, double cx) {
  const double vy = (double)r - cy, vx = (double)c - cx;
  const double nrm = sqrt(vy * vy + vx * vx) + 1e-7;
  const double oy = (vy + 1e-8) / nrm, ox = (vx + 1e-8) / nrm;  // the centroid pixel: (0.1, 0.1)
  double a = asin(oy);
  const bool xpos = ox > 0, ypos = oy > 0;
  if (!xpos) a = ypos ? M_PI - a : -M_PI - a;
  a = a + M_PI / 8;
  const double k = floor((a + M_PI) * 8 / 2 / M_PI);
  return (int)fmod(k, 8.0);  // k >= 0
}

// Thread i of workgroup (x, b) owns the network pixels 4 i .. 4 i + 3 of the workgroup's kFillPix.  VEC: H * W % 4 == 0 and
// every output 16-byte aligned (d_cls: 4-byte), so the 4 pixels exist together and every store below is one aligned vector.
template <bool VEC, class GEO>
__global__ __launch_bounds__(256) void fill_kernel(const int *gt, const int *ids, const int *count, const int *tab,
                                                    const double *cen, const GEO src, int H, int HW, int W, int T, int nc,
                                                    double sy_, double sx_, float *y_gt, unsigned char *d_cls, float *d_gt,
                                                    float *c_gt) {
  __shared__ int cat[kMaxGt], info[kMaxGt];
  __shared__ double ceny[kMaxGt], cenx[kMaxGt];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int n = clamp_count(count[b]);
  cat[tid] = tid < n ? ids[(size_t)b * kMaxGt + tid] : 0x7fffffff;
  info[tid] = tab[(size_t)b * kMaxGt + tid];
  ceny[tid] = cen[((size_t)b * 2 + 0) * kMaxGt + tid];
  cenx[tid] = cen[((size_t)b * 2 + 1) * kMaxGt + tid];
  __syncthreads();
  const long long base = (long long)blockIdx.x * kFillPix + 4 * tid;  // <= HW + kFillPix
  if (base >= HW) return;
  const Sampling sm = sampling_of(gt, src, b, H, W, sy_, sx_);
  const int *g = sm.g;
  const int Hf = sm.Hf, Wf = sm.Wf;
  const double sy = sm.sy, sx = sm.sx;
  int rank[4], cls[4], dc[4];
  bool ok[4];
  int prev_id = 0, prev_s = -1;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    rank[j] = cls[j] = -1, dc[j] = 0;
    ok[j] = base + j < HW;
    if (!ok[j]) continue;
    const int p = (int)base + j, r = p / W, c = p - r * W;
    const int id = g[(size_t)nn_src(r, sy, Hf) * Wf + nn_src(c, sx, Wf)];
    const int s = (j > 0 && id == prev_id) ? prev_s : gtid::find_slot(cat, n, id);
    prev_id = id, prev_s = s;
    if (s >= 0 && info[s] >= 0) {
      rank[j] = info[s] & 0xffff, cls[j] = info[s] >> 16;
      if (d_cls || d_gt) dc[j] = orientation_class(r, c, ceny[s], cenx[s]);
    }
  }
  const size_t px = (size_t)b * HW + base;  // this thread's first pixel among all images'
  if (y_gt) {
    float *yp = y_gt + (size_t)b * T * HW + base;
    for (int t = 0; t < T; ++t, yp += HW) {
      if (VEC) {
        *reinterpret_cast<f32x4 *>(yp) = f32x4{rank[0] == t ? 1.f : 0.f, rank[1] == t ? 1.f : 0.f, rank[2] == t ? 1.f : 0.f,
                                               rank[3] == t ? 1.f : 0.f};
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (ok[j]) yp[j] = rank[j] == t ? 1.f : 0.f;
      }
    }
  }
  if (d_cls) {
    if (VEC) {
      *reinterpret_cast<unsigned *>(d_cls + px) = (unsigned)dc[0] | (unsigned)dc[1] << 8 | (unsigned)dc[2] << 16 | (unsigned)dc[3] << 24;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (ok[j]) d_cls[px + j] = (unsigned char)dc[j];
    }
  }
  if (d_gt) {  // ins_seg_dataset.py:257-262: d_gt[..., o] = (d_cls == o)
    float *dp = d_gt + px * 8;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (!ok[j]) continue;
      if (VEC) {
#pragma unroll
        for (int h = 0; h < 2; ++h)
          *reinterpret_cast<f32x4 *>(dp + j * 8 + h * 4) = f32x4{dc[j] == 4 * h ? 1.f : 0.f, dc[j] == 4 * h + 1 ? 1.f : 0.f,
                                                                 dc[j] == 4 * h + 2 ? 1.f : 0.f, dc[j] == 4 * h + 3 ? 1.f : 0.f};
      } else {
#pragma unroll
        for (int o = 0; o < 8; ++o) dp[j * 8 + o] = dc[j] == o ? 1.f : 0.f;
      }
    }
  }
  if (c_gt) {  // ins_seg_dataset.py:216-236
    if (nc == 1) {
      float *cp = c_gt + px;
      if (VEC) {
        *reinterpret_cast<f32x4 *>(cp) = f32x4{cls[0] >= 0 ? 1.f : 0.f, cls[1] >= 0 ? 1.f : 0.f, cls[2] >= 0 ? 1.f : 0.f,
                                               cls[3] >= 0 ? 1.f : 0.f};
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (ok[j]) cp[j] = cls[j] >= 0 ? 1.f : 0.f;
      }
    } else {  // 1 + kCsClasses channels: channel 0 = 1 - max of the others = the background
      constexpr int C = 1 + gtid::kCsClasses;
      float *cp = c_gt + px * C;
      if (VEC) {  // 4 pixels x 9 channels = 9 vectors, 16-byte aligned since px % 4 == 0
#pragma unroll
        for (int q = 0; q < C; ++q) {
          f32x4 v;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int f = 4 * q + e, j = f / C, ch = f - j * C;
            v[e] = (ch == 0 ? cls[j] < 0 : cls[j] == ch - 1) ? 1.f : 0.f;
          }
          *reinterpret_cast<f32x4 *>(cp + 4 * q) = v;
        }
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (!ok[j]) continue;
#pragma unroll
          for (int ch = 0; ch < C; ++ch) cp[j * C + ch] = (ch == 0 ? cls[j] < 0 : cls[j] == ch - 1) ? 1.f : 0.f;
        }
      }
    }
  }
}

// Thread i of workgroup (x, b) owns the full-size pixels 4 i .. 4 i + 3 of the workgroup's kFillPix.
// fg has the layout of gt: [B,Hf,Wf], or flat at the same offsets.  The grid covers the largest image; a workgroup beyond
// its own image's pixels leaves.
template <class GEO>
__global__ __launch_bounds__(256) void fg_full_kernel(const int *gt, const GEO src, int dataset, unsigned char *fg) {
  const geo::Image im = src.at(blockIdx.y);
  const unsigned HWf = (unsigned)im.h * (unsigned)im.w;  // < 2^31
  const int vec_ok = im.vec;
  const unsigned long long base = (unsigned long long)blockIdx.x * kFillPix + 4 * threadIdx.x;
  if (base >= HWf) return;
  const int *g = gt + im.off + base;
  unsigned char *o = fg + im.off + base;
  int cls;
  if (vec_ok) {  // the 4 pixels exist together (uniform: HWf % 4 == 0; ragged: w % 4 == 0), gt 16-byte and fg 4-byte aligned
    const i32x4 v = __builtin_nontemporal_load(reinterpret_cast<const i32x4 *>(g));
    unsigned w = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) w |= (accept(dataset, v[j], cls) ? 1u : 0u) << (8 * j);
    *reinterpret_cast<unsigned *>(o) = w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (base + j < HWf) o[j] = accept(dataset, g[j], cls) ? 1 : 0;
  }
}

inline bool plane_ok(int H, int W) { return H > 0 && W > 0 && (long long)H * W < (1ll << 31); }
inline int mom_wgs(int B, long long HW) {
  const long long tiles = (HW + 255) / 256;
  const int want = kMomWgs / B > 0 ? kMomWgs / B : 1;
  return tiles < want ? (int)tiles : want;
}
inline size_t part_bytes(int B, int H, int W) { return (size_t)B * mom_wgs(B, (long long)H * W) * 3 * kMaxGt * sizeof(u64); }
inline size_t cen_bytes(int B) { return (size_t)B * 2 * kMaxGt * sizeof(double); }
inline size_t tab_bytes(int B) { return (size_t)B * kMaxGt * sizeof(int); }

// The stage's launches behind the argument checks, for either geometry source.  src_fg: the source with fg_full's vector
// rule (its own alignment needs); max_HWf: the largest image's pixels (fg_full's grid); sy, sx: the uniform form's scales.
template <class GEO>
int launch_stage(const char *who, const int *gt_ids, const GEO &src, const GEO &src_fg, long long max_HWf, const int *ids,
                 const int *count, int B, int H, int W, int T, int dataset, double sy, double sx, void *ws, int *num_obj,
                 float *s_gt, int *inst_id, int *area, int *sem_cls, float *y_gt, unsigned char *d_cls, float *d_gt, float *c_gt,
                 unsigned char *fg_gt_full, hipStream_t st) {
  char what[96];
  const auto status = [&](const char *stage) {
    snprintf(what, sizeof(what), "%s (%s)", who, stage);
    return launch_status(what);
  };
  const int HW = H * W;
  const bool want_fill = y_gt || d_cls || d_gt || c_gt;
  if (want_fill || num_obj || s_gt || inst_id || area || sem_cls) {
    u64 *part = static_cast<u64 *>(ws);
    double *cen = reinterpret_cast<double *>(static_cast<char *>(ws) + part_bytes(B, H, W));
    int *tab = reinterpret_cast<int *>(reinterpret_cast<char *>(cen) + cen_bytes(B));
    const int nwg = mom_wgs(B, HW);
    hipLaunchKernelGGL(moments_kernel<GEO>, dim3(nwg, B), dim3(256), 0, st, gt_ids, ids, count, src, H, HW, W, sy, sx,
                       (int)(((long long)HW + 255) / 256), part);
    if (int rc = status("moments")) return rc;
    hipLaunchKernelGGL(rank_kernel, dim3(B), dim3(256), 0, st, part, nwg, ids, count, T, dataset, num_obj, s_gt, inst_id, area,
                       sem_cls, tab, cen);
    if (int rc = status("rank")) return rc;
    if (want_fill) {
      const int nc = dataset == RA_LABELS_CITYSCAPES ? 1 + gtid::kCsClasses : 1;
      const uintptr_t al = reinterpret_cast<uintptr_t>(y_gt) | reinterpret_cast<uintptr_t>(d_gt) | reinterpret_cast<uintptr_t>(c_gt);
      const bool vec = HW % 4 == 0 && (al & 15) == 0 && (reinterpret_cast<uintptr_t>(d_cls) & 3) == 0;
      const dim3 grid((unsigned)(((long long)HW + kFillPix - 1) / kFillPix), B);
      if (vec)
        hipLaunchKernelGGL((fill_kernel<true, GEO>), grid, dim3(256), 0, st, gt_ids, ids, count, tab, cen, src, H, HW, W, T, nc, sy,
                           sx, y_gt, d_cls, d_gt, c_gt);
      else
        hipLaunchKernelGGL((fill_kernel<false, GEO>), grid, dim3(256), 0, st, gt_ids, ids, count, tab, cen, src, H, HW, W, T, nc,
                           sy, sx, y_gt, d_cls, d_gt, c_gt);
      if (int rc = status("fill")) return rc;
    }
  }
  if (fg_gt_full) {
    hipLaunchKernelGGL(fg_full_kernel<GEO>, dim3((unsigned)((max_HWf + kFillPix - 1) / kFillPix), B), dim3(256), 0, st, gt_ids,
                       src_fg, dataset, fg_gt_full);
    if (int rc = status("fg_full")) return rc;
  }
  return 0;
}

}  // namespace lab
}  // namespace ra

using namespace ra;

extern "C" size_t ra_labels_workspace_bytes(int B, int H, int W) {
  if (B <= 0 || !lab::plane_ok(H, W)) return 0;
  return lab::part_bytes(B, H, W) + lab::cen_bytes(B) + lab::tab_bytes(B);
}

extern "C" int ra_labels_assemble_i32(const int *gt_ids, const int *ids, const int *count, int B, int Hf, int Wf, int H, int W,
                                      int T, int dataset, void *ws, size_t ws_bytes, int *num_obj, float *s_gt, int *inst_id,
                                      int *area, int *sem_cls, float *y_gt, unsigned char *d_cls, float *d_gt, float *c_gt,
                                      unsigned char *fg_gt_full, void *stream) {
  if (!gt_ids || !ids || !count || !ws || B <= 0 || (reinterpret_cast<uintptr_t>(ws) & 7))
    return fail(RA_E_INVALID, "ra_labels_assemble_i32: bad argument");
  if (T < 1 || T > lab::kMaxT || !lab::plane_ok(Hf, Wf) || H < 1 || H > Hf || W < 1 || W > Wf || B > 65535 ||
      (dataset != RA_LABELS_PLAIN && dataset != RA_LABELS_CITYSCAPES))
    return fail(RA_E_SHAPE, "ra_labels_assemble_i32: T=%d ids %dx%d -> %dx%d B=%d dataset=%d (1 <= T <= %d, 1 <= H <= Hf, 1 <= W <= Wf, "
                "Hf * Wf < 2^31, B <= 65535)", T, Hf, Wf, H, W, B, dataset, lab::kMaxT);
  if (ws_bytes < ra_labels_workspace_bytes(B, H, W)) return fail(RA_E_WORKSPACE, "ra_labels_assemble_i32: workspace");
  const long long HWf = (long long)Hf * Wf;
  const double sy = 1.0 / ((double)H / (double)Hf), sx = 1.0 / ((double)W / (double)Wf);
  const int vec_fg = HWf % 4 == 0 && (reinterpret_cast<uintptr_t>(gt_ids) & 15) == 0 && (reinterpret_cast<uintptr_t>(fg_gt_full) & 3) == 0;
  return lab::launch_stage("ra_labels_assemble_i32", gt_ids, geo::Uniform{Hf, Wf, 0}, geo::Uniform{Hf, Wf, vec_fg}, HWf, ids, count, B,
                           H, W, T, dataset, sy, sx, ws, num_obj, s_gt, inst_id, area, sem_cls, y_gt, d_cls, d_gt, c_gt, fg_gt_full,
                           as_stream(stream));
}

extern "C" int ra_labels_assemble_ragged_i32(const int *gt_ids, size_t total, const ra_image_geo *geo, ra_image_geo *geo_dev,
                                             const int *ids, const int *count, int B, int H, int W, int T, int dataset, void *ws,
                                             size_t ws_bytes, int *num_obj, float *s_gt, int *inst_id, int *area, int *sem_cls,
                                             float *y_gt, unsigned char *d_cls, float *d_gt, float *c_gt,
                                             unsigned char *fg_gt_full, void *stream) {
  const char *who = "ra_labels_assemble_ragged_i32";
  if (!gt_ids || !geo || !geo_dev || !ids || !count || !ws || B <= 0 || (reinterpret_cast<uintptr_t>(ws) & 7))
    return fail(RA_E_INVALID, "%s: bad argument", who);
  if (T < 1 || T > lab::kMaxT || !lab::plane_ok(H, W) || B > 65535 || (dataset != RA_LABELS_PLAIN && dataset != RA_LABELS_CITYSCAPES))
    return fail(RA_E_SHAPE, "%s: T=%d -> %dx%d B=%d dataset=%d (1 <= T <= %d, H, W >= 1, H * W < 2^31, B <= 65535)", who, T, H, W, B,
                dataset, lab::kMaxT);
  if (int rc = geo::check(who, geo, B, total, (1ll << 31) - 1, "h * w < 2^31")) return rc;
  for (int b = 0; b < B; ++b)
    if (H > geo[b].h || W > geo[b].w)
      return fail(RA_E_SHAPE, "%s: image %d is %d x %d, below the network size %d x %d (1 <= H <= h, 1 <= W <= w for every image)",
                  who, b, geo[b].h, geo[b].w, H, W);
  if (ws_bytes < ra_labels_workspace_bytes(B, H, W)) return fail(RA_E_WORKSPACE, "%s: workspace", who);
  hipStream_t st = as_stream(stream);
  if (int rc = geo::upload(who, geo, geo_dev, B, st)) return rc;
  const int vec_fg = (reinterpret_cast<uintptr_t>(gt_ids) & 15) == 0 && (reinterpret_cast<uintptr_t>(fg_gt_full) & 3) == 0;
  return lab::launch_stage(who, gt_ids, geo::Ragged{geo_dev, 0}, geo::Ragged{geo_dev, vec_fg}, geo::max_pixels(geo, B), ids, count,
                           B, H, W, T, dataset, 0.0, 0.0, ws, num_obj, s_gt, inst_id, area, sem_cls, y_gt, d_cls, d_gt, c_gt,
                           fg_gt_full, st);
}
