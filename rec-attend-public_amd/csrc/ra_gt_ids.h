// What the kernels that read *_instanceIds.png values share: the Cityscapes "thing" labels and the catalogue lookup.
#pragma once
#include "ra_common.h"

namespace ra {
namespace gtid {

// analysis.py:203-210 (CITYSCAPES_LABELS): person, rider, car, truck, bus, train, motorcycle, bicycle — the labels whose
// trainId is positive in data_api/cityscapes.py; a label's position is its semantic class
constexpr int kCsClasses = 8;
__host__ __device__ __forceinline__ int cs_label_id(int cls) {
  constexpr int ids[kCsClasses] = {24, 25, 26, 27, 28, 31, 32, 33};
  return ids[cls];
}
// the position of label id `label` in that tuple, -1 when it is not one of them
__host__ __device__ __forceinline__ int cs_class_of(int label) {
  int cls = -1;
#pragma unroll
  for (int k = 0; k < kCsClasses; ++k) cls = cs_label_id(k) == label ? k : cls;
  return cls;
}

// the slot of id in the sorted catalogue cat[0, n), -1 when it is not there
__device__ __forceinline__ int find_slot(const int *cat, int n, int id) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (cat[mid] < id) lo = mid + 1;
    else hi = mid;
  }
  return lo < n && cat[lo] == id ? lo : -1;
}

}  // namespace gtid
}  // namespace ra
