// Where the images of a batch of full-size planes lie: the two geometry sources the kernels that work at the labels' own size
// are templated over, and the host-side check of a ragged table (include/recattend.h, ra_image_geo).
//
//   Uniform   B images of ONE size back to back, [B,h,w]: image b starts at element b * h * w.  Everything is a kernel argument.
//   Ragged    B images of their own sizes in one flat buffer, rows packed with pitch w: image b is tab[b].  tab is indexed by
//             blockIdx alone, so the entry is ONE scalar load per workgroup and h, w, offset live in scalar registers, as the
//             kernel arguments of the uniform form do.
//
// vec says whether a lane may fetch its 4 consecutive elements of a row as one vector (16 bytes of int32 ids, 4 bytes of uint8
// labels).  Uniform: the launch decides (its own rule, unchanged).  Ragged: per image — the base pointers are aligned (the
// launch's share, Ragged::vec) and w % 4 == 0 and offset % 4 == 0 (the image's share); an image that misses takes element loads
// and its neighbours are unaffected.  The load width touches no arithmetic.
#pragma once
#include "ra_common.h"

namespace ra {
namespace geo {

struct Image {
  long long off;  // first element in the buffer
  int h, w;
  int vec;
};

struct Uniform {
  static constexpr bool kRagged = false;
  int h, w, vec;
  __device__ __forceinline__ Image at(int b) const { return Image{(long long)b * h * w, h, w, vec}; }
};

struct Ragged {
  static constexpr bool kRagged = true;
  const ra_image_geo *tab;
  int vec;
  __device__ __forceinline__ Image at(int b) const {
    const ra_image_geo g = tab[b];  // b = a blockIdx: a scalar load
    return Image{g.offset, g.h, g.w, (vec && g.w % 4 == 0 && g.offset % 4 == 0) ? 1 : 0};
  }
};

// The largest h * w of a table (0 for an empty or NULL one): the grid of a ragged launch is sized from it.
inline long long max_pixels(const ra_image_geo *g, int B) {
  long long m = 0;
  for (int b = 0; g && b < B; ++b) {
    const long long p = g[b].h > 0 && g[b].w > 0 ? (long long)g[b].h * g[b].w : 0;
    m = p > m ? p : m;
  }
  return m;
}

// 0, or RA_E_SHAPE with a message that names the image: h, w >= 1; h * w <= cap (`cap_text` says why); image b starts at or
// behind the end of image b - 1 (the first at or behind 0) and ends within `total` elements.
inline int check(const char *who, const ra_image_geo *g, int B, size_t total, long long cap, const char *cap_text) {
  long long end = 0;
  for (int b = 0; b < B; ++b) {
    if (g[b].h < 1 || g[b].w < 1) return fail(RA_E_SHAPE, "%s: image %d is %d x %d (h, w >= 1)", who, b, g[b].h, g[b].w);
    const long long px = (long long)g[b].h * g[b].w;
    if (px > cap) return fail(RA_E_SHAPE, "%s: image %d is %d x %d (%s)", who, b, g[b].h, g[b].w, cap_text);
    if (g[b].offset < end)
      return fail(RA_E_SHAPE, "%s: image %d starts at element %lld, inside image %d which ends at %lld (images in ascending order, "
                  "no overlap)", who, b, g[b].offset, b - 1, end);
    end = g[b].offset + px;
    if ((unsigned long long)end > (unsigned long long)total)
      return fail(RA_E_SHAPE, "%s: image %d (%d x %d at element %lld) ends at %lld, beyond the buffer's %llu elements", who, b,
                  g[b].h, g[b].w, g[b].offset, end, (unsigned long long)total);
  }
  return 0;
}

// The table onto the device, on the stream ahead of the kernels that read it.
inline int upload(const char *who, const ra_image_geo *g, ra_image_geo *dev, int B, hipStream_t st) {
  if (hipMemcpyAsync(dev, g, (size_t)B * sizeof(ra_image_geo), hipMemcpyHostToDevice, st) != hipSuccess) return launch_status(who);
  return 0;
}

}  // namespace geo
}  // namespace ra
