// What the two fused-pair sources share (ra_conv_pair.hip: the generic pair and the plan query; ra_conv_pair8.hip: the N-packed
// first pair with its cache): the kernel argument record, the host code that fills it, and the declarations through which
// ra_conv_pair_f32 and ra_conv_pair_plan reach the N-packed launches.
#pragma once
#include <cstdint>
#include <initializer_list>

#include "ra_common.h"

namespace ra {
namespace cpair {

// One record for both kernel families.  The N-packed kernels read it as their first kernel argument: its layout is fixed.
struct PArgs {
  const float *src;
  float *y;
  const float *wpA, *scA, *shA, *wpB, *scB, *shB;
  int C0, Hs, Ws, H, W, ups;
  int CoutAP, CoutB, CoutBP, poolB, Ho, Wo, reluA, reluB;
  const float *plane;  // optional [B,Hs,Ws] plane replacing input channel plane_chan (the canvas)
  int plane_chan;
  int bytes0, bytes_p;  // tensor sizes for the buffer descriptors (each < 2 GiB)
  const float *cache;   // conv_pair8 CACHED form: layer A's timestep-invariant partial sums
  int cache_rows, cache_gx, bytes_c;
  int bytes_y;  // conv_pair8: size of y for its buffer descriptor (< 2 GiB whenever the input is)
  int xcd_map;  // conv_pair8: 1 = each XCD (workgroup id mod 8) walks its own contiguous eighth of the tiles
  // conv_pair8, un-cached form only: a constant fill of another buffer rides on the launch (the decode loop's
  // once-per-forward prefill of y_out, 134 MB at cfg2: this kernel is MFMA-bound and leaves HBM idle, so the
  // stores, a few per thread and tile, cost nothing on the timeline — as a launch of its own they cost 28 us)
  float *rider_dst;
  int rider_quads;  // float4 groups to write (rider_dst 16-byte aligned, < 2 GiB)
  float rider_val;
  unsigned *tickets;  // conv_pair8: this launch's slot of tile-ticket pools (ra_common.h), nullptr = the static tile walk
};

template <int N>
struct vec_of {
  typedef float type __attribute__((ext_vector_type(N)));
};

// A launch (plan == nullptr) that lacks one of its pointers; a plan query follows none.
inline bool missing_pointer(const int *plan, std::initializer_list<const void *> ptrs) {
  if (plan) return false;
  for (const void *p : ptrs)
    if (!p) return true;
  return false;
}

// The launch arguments every pair entry point fills alike: layer A over src [B,Hs,Ws,Cin] (the stride-2 transposed conv with
// upsampleA), layer B with pool poolB.  bytes0, the cache and the rider stay zero: each entry point sets what its form reads.
inline PArgs pair_args(const float *src, int Cin, int B, int Hs, int Ws, int upsampleA, const float *wpA, const float *scaleA,
                       const float *shiftA, int CoutA, int reluA, const float *wpB, const float *scaleB, const float *shiftB,
                       int CoutB, int reluB, int poolB, const float *plane, int plane_chan, float *y) {
  PArgs a{};
  a.src = src;
  a.y = y;
  a.wpA = wpA;
  a.scA = scaleA;
  a.shA = shiftA;
  a.wpB = wpB;
  a.scB = scaleB;
  a.shB = shiftB;
  a.C0 = Cin;
  a.Hs = Hs;
  a.Ws = Ws;
  a.ups = upsampleA ? 1 : 0;
  a.H = Hs * (1 + a.ups);
  a.W = Ws * (1 + a.ups);
  a.CoutAP = ra_conv_cout_padded(CoutA);
  a.CoutB = CoutB;
  a.CoutBP = ra_conv_cout_padded(CoutB);
  a.poolB = poolB;
  a.Ho = a.H / poolB;
  a.Wo = a.W / poolB;
  a.reluA = reluA;
  a.reluB = reluB;
  a.plane = plane;
  a.plane_chan = plane_chan;
  a.bytes_p = (int)((size_t)B * Hs * Ws * 4);
  return a;
}

void cache_dims(int H, int W, int &rows, int &ngx);  // ra_conv_pair8.hip: rows and column groups of the cache of an H x W image

// ... and layer A's cached partial sums, for the two forms of the first pair that write / read them.  0, or `what`'s error.
inline int pair_args_cache(PArgs &a, const float *cache, int B, const char *what) {
  a.cache = cache;
  cache_dims(a.H, a.W, a.cache_rows, a.cache_gx);
  const size_t cb = (size_t)B * a.cache_rows * a.cache_gx * 64 * sizeof(float);
  if (cb >= (1ull << 31)) return fail(RA_E_SHAPE, "%s: cache exceeds 2 GiB", what);
  a.bytes_c = (int)cb;
  return 0;
}

// The N-packed first pair (ra_conv_pair8.hip), as the generic entry and the plan query reach it; plan != nullptr: the same checks
// and choices, ending in a record instead of a launch.
int launch_npacked(const PArgs &a, int B, hipStream_t st, int *plan);  // a.C0 = 4 | 8, un-cached
int fill_cache_entry(const float *src, const float *plane, int plane_chan, int B, int H, int W, const float *wpA, const float *scaleA,
                     const float *shiftA, int reluA, const float *wpB, const float *scaleB, const float *shiftB, int CoutB, int reluB,
                     float *cache, float *y, float *fill_dst, size_t fill_floats, float fill_value, void *stream, int *plan);
int cached_entry(const float *cache, const float *plane, int plane_chan, int B, int H, int W, const float *wpA, const float *scaleA,
                 const float *shiftA, int reluA, const float *wpB, const float *scaleB, const float *shiftB, int CoutB, int reluB,
                 float *y, void *stream, int *plan);

}  // namespace cpair
}  // namespace ra
