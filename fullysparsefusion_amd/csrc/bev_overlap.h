// The BEV overlap of two boxes (x1, y1, x2, y2, yaw) and their IoU, shared by K20's pair kernels (nms.hip) and by the host
// program tests/host/bev_overlap_check.cpp, which runs the same text under the address / undefined-behaviour sanitizers.
// No HIP header is needed: with hipcc the functions are __host__ __device__, with a plain C++ compiler they are inline.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define FSF_BEV_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define FSF_BEV_FN static inline
#endif

namespace fsf {

// Capacity of the clip polygon.  In exact arithmetic the polygon is convex and never has more than 8 vertices; in fp32 a corner
// of a coincident box can land one ulp outside a side and a near-collinear edge then crosses it twice.  Worst count seen by the
// host check (tests/host/bev_overlap_check.cpp: the degenerate families + 2 000 000 identical pairs, -ffp-contract=off): 10 (BEV_CLIP_WORST_SEEN).
// What the comparisons could do at worst: a pass over a cyclic list of n vertices keeps the `in` ones and adds one per in/out
// transition, at most 2 min(in, out) of them, i.e. n + floor(n / 2) vertices: 4 -> 6 -> 9 -> 13 -> 19.  16 slots cover what
// fp32 produces with room to spare and keep the arrays in registers (4 x 16 floats: the pair kernels stay at 112-133 VGPRs;
// 20 slots took 182-202 and left two waves per SIMD).  Every append is guarded, so no input - NaN and inf included - can write
// past a slot; a polygon that did reach the capacity would lose its last vertices, not its neighbours' memory.
constexpr int BEV_CLIP_CAP = 16;
constexpr int BEV_CLIP_WORST_SEEN = 10;  // the host check fails when it finds more: then this line and the capacity are due for a look

// `max_vertices` (host checks only; nullptr on the device): raised to the largest vertex count a pass produced.
FSF_BEV_FN float rect_overlap_rotated(const float* a, const float* b, int* max_vertices = nullptr) {
  // B frame: origin at B's centre, axes along B's sides
  const float bcx = 0.5f * (b[0] + b[2]), bcy = 0.5f * (b[1] + b[3]);
  const float bhx = 0.5f * (b[2] - b[0]), bhy = 0.5f * (b[3] - b[1]);
  const float acx = 0.5f * (a[0] + a[2]), acy = 0.5f * (a[1] + a[3]);
  const float ahx = 0.5f * (a[2] - a[0]), ahy = 0.5f * (a[3] - a[1]);
  if (!(bhx > 0.f) || !(bhy > 0.f) || !(ahx > 0.f) || !(ahy > 0.f)) return 0.f;
  const float ca = cosf(a[4]), sa = sinf(a[4]), cb = cosf(b[4]), sb = sinf(b[4]);
  // Upstream's corner rotation (iou3d rotate_around_center, the mmdet3d 0.x yaw sense, the same one K17's
  // lidar_to_local_coords implies): corner = centre + M(yaw) * offset with M = [[cos, sin], [-sin, cos]].
  // Polygon = A's corners in the world, then into B's frame with M(yaw_b)^T.
  float px[BEV_CLIP_CAP], py[BEV_CLIP_CAP], qx[BEV_CLIP_CAP], qy[BEV_CLIP_CAP];
  const float ox[4] = {-ahx, ahx, ahx, -ahx}, oy[4] = {-ahy, -ahy, ahy, ahy};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float wx = acx + ca * ox[k] + sa * oy[k] - bcx;
    const float wy = acy - sa * ox[k] + ca * oy[k] - bcy;
    px[k] = cb * wx - sb * wy;
    py[k] = sb * wx + cb * wy;
  }
  int n = 4;
  // clip against x <= bhx, x >= -bhx, y <= bhy, y >= -bhy
#pragma unroll
  for (int side = 0; side < 4; ++side) {
    const float lim = (side < 2) ? bhx : bhy;
    const float sgn = (side & 1) ? -1.f : 1.f;
    int m = 0;
    for (int k = 0; k < n; ++k) {
      const int k2 = (k + 1 == n) ? 0 : k + 1;
      const float c0 = sgn * ((side < 2) ? px[k] : py[k]);
      const float c1 = sgn * ((side < 2) ? px[k2] : py[k2]);
      const bool in0 = c0 <= lim, in1 = c1 <= lim;
      if (in0 && m < BEV_CLIP_CAP) {
        qx[m] = px[k];
        qy[m] = py[k];
        ++m;
      }
      if (in0 != in1 && m < BEV_CLIP_CAP) {
        const float t = (lim - c0) / (c1 - c0);
        qx[m] = px[k] + t * (px[k2] - px[k]);
        qy[m] = py[k] + t * (py[k2] - py[k]);
        ++m;
      }
    }
    n = m;
    if (max_vertices && n > *max_vertices) *max_vertices = n;
    for (int k = 0; k < n; ++k) {
      px[k] = qx[k];
      py[k] = qy[k];
    }
    if (n < 3) return 0.f;
  }
  float area = 0.f;
  for (int k = 1; k + 1 < n; ++k)
    area += (px[k] - px[0]) * (py[k + 1] - py[0]) - (px[k + 1] - px[0]) * (py[k] - py[0]);
  return 0.5f * fabsf(area);
}

FSF_BEV_FN float rect_overlap_normal(const float* a, const float* b) {
  const float l = fmaxf(a[0], b[0]), r = fminf(a[2], b[2]);
  const float t = fmaxf(a[1], b[1]), d = fminf(a[3], b[3]);
  return fmaxf(r - l, 0.f) * fmaxf(d - t, 0.f);
}

FSF_BEV_FN float iou_bev(const float* a, const float* b, int rotated, int* max_vertices = nullptr) {
  const float sa = (a[2] - a[0]) * (a[3] - a[1]);
  const float sb = (b[2] - b[0]) * (b[3] - b[1]);
  const float ov = rotated ? rect_overlap_rotated(a, b, max_vertices) : rect_overlap_normal(a, b);
  return ov / fmaxf(sa + sb - ov, 1e-8f);
}

}  // namespace fsf
