// The tap arithmetic of the bilinear image-feature gather, shared by its forward (K13b, project.hip) and its backward (K13c,
// project_bwd.hip): FSF.prj_points_2d (FSF.py:169-200: fma chain, depth / image validity) followed by
// F.grid_sample(mode='bilinear', align_corners=False, padding_mode='zeros')'s corner rule.  ONE definition, so that both kernels form
// the same bits (the library is built with -ffp-contract=off: every product, sum and difference below is rounded on its own).
#pragma once
#include "common.h"

namespace fsf {

// pts_4d @ lidar2img^T for one output row: ((x*m0 + y*m1) + z*m2) + m3 as an fma chain in k order,
// which is what the CPU sgemm micro-kernel of the in-container reference evaluates (see oracle/project.py).
__device__ __forceinline__ float proj_row(const float* m, float x, float y, float z) {
  float acc = __fmul_rn(x, m[0]);
  acc = __fmaf_rn(y, m[1], acc);
  acc = __fmaf_rn(z, m[2], acc);
  acc = __fmaf_rn(1.0f, m[3], acc);
  return acc;
}

// One (point, camera): `valid` = the projection lands inside the image; (x0, y0) the top-left corner (x0 in [-1, Wf - 1], y0 in
// [-1, Hf - 1] when valid); wx1 / wy1 the fractions, wx0 = 1 - wx1, wy0 = 1 - wy1; w_dydx = wx * wy, zero when the corner is outside
// the map or the projection is invalid; (xa, ya) / (xb, yb) the corners clamped into the map.
struct BilinearTaps {
  bool valid;
  int x0, y0;
  float wx1, wy1;
  float w00, w01, w10, w11;
  int xa, xb, ya, yb;
};

// m: rows 0..2 of the camera's 4x4 (12 floats); fw, fh: the image size the projection normalises by
__device__ __forceinline__ BilinearTaps bilinear_taps(const float* m, float x, float y, float z, float fw, float fh, int Hf, int Wf) {
  BilinearTaps t;
  float px = proj_row(m, x, y, z), py = proj_row(m + 4, x, y, z), pz = proj_row(m + 8, x, y, z);
  const bool depth_valid = pz > 1e-3f;
  pz = fminf(fmaxf(pz, 1e-5f), 1e5f);
  px = __fdiv_rn(__fdiv_rn(px, pz), fw);
  py = __fdiv_rn(__fdiv_rn(py, pz), fh);
  const float gx = __fmul_rn(__fsub_rn(px, 0.5f), 2.0f), gy = __fmul_rn(__fsub_rn(py, 0.5f), 2.0f);
  const bool valid = depth_valid && gx > -1.0f && gx < 1.0f && gy > -1.0f && gy < 1.0f;
  // grid_sample, align_corners = False
  const float ix = ((gx + 1.0f) * (float)Wf - 1.0f) * 0.5f, iy = ((gy + 1.0f) * (float)Hf - 1.0f) * 0.5f;
  const float x0f = floorf(ix), y0f = floorf(iy);
  const float wx1 = ix - x0f, wy1 = iy - y0f, wx0 = 1.0f - wx1, wy0 = 1.0f - wy1;
  const int x0 = (int)x0f, y0 = (int)y0f;
  const bool inx0 = x0 >= 0 && x0 < Wf, inx1 = x0 + 1 >= 0 && x0 + 1 < Wf;
  const bool iny0 = y0 >= 0 && y0 < Hf, iny1 = y0 + 1 >= 0 && y0 + 1 < Hf;
  t.w00 = valid && inx0 && iny0 ? wx0 * wy0 : 0.0f;
  t.w01 = valid && inx1 && iny0 ? wx1 * wy0 : 0.0f;
  t.w10 = valid && inx0 && iny1 ? wx0 * wy1 : 0.0f;
  t.w11 = valid && inx1 && iny1 ? wx1 * wy1 : 0.0f;
  t.xa = min(max(x0, 0), Wf - 1);
  t.xb = min(max(x0 + 1, 0), Wf - 1);
  t.ya = min(max(y0, 0), Hf - 1);
  t.yb = min(max(y0 + 1, 0), Hf - 1);
  t.valid = valid;
  t.x0 = x0;
  t.y0 = y0;
  t.wx1 = wx1;
  t.wy1 = wy1;
  return t;
}

}  // namespace fsf
