// The pinned containment test of mmdet3d 0.x points_in_boxes_gpu (check_pt_in_box3d), shared by K35a (points -> segmentation
// targets, seg_loss.hip) and K36a (cluster centres -> query-head targets, cluster_loss.hip).  See include/fsf_hip.h, section K35.
#pragma once
#include "common.h"

namespace fsf {

constexpr int BOX_WORDS = 8;  // (cx, cy, cz, half_w, half_l, half_h, cosa, sina)

// One box's constants: cz = f32(z + h / 2), half sizes, cos / sin(-yaw) in float64 rounded once.
__device__ __forceinline__ void box_constants(float x, float y, float z, float w, float l, float h, float rz, float* __restrict__ t) {
  const double yaw = -(double)rz;
  t[0] = x;
  t[1] = y;
  t[2] = __fadd_rn(z, h * 0.5f);
  t[3] = w * 0.5f;
  t[4] = l * 0.5f;
  t[5] = h * 0.5f;
  t[6] = (float)cos(yaw);
  t[7] = (float)sin(yaw);
}

// Index of the first box in [k0, k1) with a label >= 0 that contains (px, py, pz), -1 when none.  Every product and sum is a
// separately rounded f32 operation; the z test is |z - cz| > h / 2 and the footprint test is strict on all four sides.
__device__ __forceinline__ int first_box_containing(float px, float py, float pz, const float* __restrict__ table,
                                                    const int32_t* __restrict__ box_labels, int k0, int k1) {
  for (int k = k0; k < k1; ++k) {
    if (box_labels[k] < 0) continue;  // dropped GT rows (the reference filters them before points_in_boxes)
    const float* t = table + (int64_t)k * BOX_WORDS;
    if (fabsf(__fsub_rn(pz, t[2])) > t[5]) continue;
    const float sx = __fsub_rn(px, t[0]), sy = __fsub_rn(py, t[1]);
    const float cosa = t[6], sina = t[7];
    const float lx = __fadd_rn(__fmul_rn(sx, cosa), __fmul_rn(sy, -sina));
    const float ly = __fadd_rn(__fmul_rn(sx, sina), __fmul_rn(sy, cosa));
    if (lx > -t[4] && lx < t[4] && ly > -t[3] && ly < t[3]) return k;
  }
  return -1;
}

}  // namespace fsf
