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

// The label ids of helpers/labels.py run from 0 to 33 (its -1, license plate, cannot occur in an image).
constexpr int kCsLabelIds = 34;
// The instance category of a label as evalPixelLevelSemanticLabeling.py:182-200 builds it — a category all of whose labels
// have instances: 1 = human {24, 25}, 2 = vehicle {26 .. 33}, caravan (29) and trailer (30) included; 0 = neither.
__host__ __device__ __forceinline__ int cs_instance_category(int label) {
  return label == 24 || label == 25 ? 1 : (label >= 26 && label <= 33 ? 2 : 0);
}
// the label of a value of *_instanceIds.png: the value itself below 1000, else value / 1000
__host__ __device__ __forceinline__ int cs_label_of_id(int id) { return id < 1000 ? id : id / 1000; }

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
