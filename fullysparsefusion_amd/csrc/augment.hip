// K33: test-time augmentation on the device — see include/fsf_hip.h.
//   fsf_augment_points      (K33a): one assembled cloud -> A augmented clouds in one scan launch: rotation, scale, BEV flips on
//                                   xyz (GlobalRotScaleTrans then RandomFlip3D), the strict PointsRangeFilter test on the
//                                   AUGMENTED xyz, stable compaction; feature and no-aug columns copied unchanged
//   fsf_aug_boxes_map_back  (K33b): the concatenated per-pass boxes mapped back to the un-augmented frame (undo vertical flip,
//                                   horizontal flip, scale, rotation) + the NMS form of their BEV boxes + class-major scores, the
//                                   inputs of fsf_class_rank_desc / fsf_nms_bev_multiclass_capped / fsf_nms_select (K24 / K20)
// Arithmetic is pinned: every product and sum is rounded on its own (__fmul_rn / __fadd_rn, no FMA
// contraction), in the order the host classes of datasets/pipelines.py and core/bbox.py evaluate them.
#include "common.h"
#include "scan.h"

namespace fsf {

constexpr int AUG_MAX = 32;
constexpr float AUG_PI = 3.14159265358979323846f;  // np.pi as an fp32 scalar operand

struct AugDesc {
  float c, s, scale, theta;  // cos / sin of the fp32 angle (host torch.cos / torch.sin), scale, the angle itself (K33b's yaw)
  int rot, flip_h, flip_v;   // rot = 0: the angle is exactly zero and the rotation is not evaluated (identity, bit for bit)
};

struct AugArgs {
  const float* in;
  float* out;
  int64_t* offsets;
  int64_t n;
  int cols, naug, use_range;
  float range[6];
  AugDesc d[AUG_MAX];
};

// forward transform of points, host order: rotation, scale (GlobalRotScaleTrans), horizontal then vertical flip (RandomFlip3D)
__device__ __forceinline__ void aug_forward(const AugDesc& d, float& x, float& y, float& z) {
  if (d.rot) {
    const float xr = __fsub_rn(__fmul_rn(x, d.c), __fmul_rn(y, d.s));
    const float yr = __fadd_rn(__fmul_rn(x, d.s), __fmul_rn(y, d.c));
    x = xr;
    y = yr;
  }
  x = __fmul_rn(x, d.scale);
  y = __fmul_rn(y, d.scale);
  z = __fmul_rn(z, d.scale);
  if (d.flip_h) y = -y;
  if (d.flip_v) x = -x;
}

__device__ __forceinline__ bool aug_row(const AugArgs& a, int64_t i, int k, float (&xyz)[3]) {
  const float* p = a.in + (i - (int64_t)k * a.n) * a.cols;
  xyz[0] = p[0]; xyz[1] = p[1]; xyz[2] = p[2];
  aug_forward(a.d[k], xyz[0], xyz[1], xyz[2]);
  return !a.use_range || (xyz[0] > a.range[0] && xyz[1] > a.range[1] && xyz[2] > a.range[2] && xyz[0] < a.range[3] &&
                          xyz[1] < a.range[4] && xyz[2] < a.range[5]);
}

struct AugIn {
  const AugArgs* ap;
  __device__ uint32_t operator()(int64_t i) const {
    const AugArgs& a = *ap;
    float xyz[3];
    return aug_row(a, i, (int)(i / a.n), xyz) ? 1u : 0u;
  }
};

struct AugOut {
  const AugArgs* ap;
  __device__ void operator()(int64_t i, uint32_t pos, uint32_t keep) const {
    const AugArgs& a = *ap;
    const int k = (int)(i / a.n);
    const int64_t r = i - (int64_t)k * a.n;
    if (r == a.n - 1) a.offsets[k + 1] = (int64_t)pos + keep;  // end of augmentation k's rows in the concatenated output
    if (!keep) return;
    float xyz[3];
    aug_row(a, i, k, xyz);
    const float* p = a.in + r * a.cols;
    float* o = a.out + (int64_t)pos * a.cols;
    o[0] = xyz[0]; o[1] = xyz[1]; o[2] = xyz[2];
    for (int c = 3; c < a.cols; ++c) o[c] = p[c];  // features and the no-aug xyz (SaveNoAugPoints) unchanged
  }
};

// K33b: undo, in this order, vertical flip, horizontal flip, scale (x 1/s), rotation (by -theta); velocity columns 7, 8 follow
// the centre, yaw follows mmdet3d 0.x's LiDAR boxes
__global__ void __launch_bounds__(256)
    aug_map_back_kernel(const float* __restrict__ boxes, int64_t box_stride, int D, const float* __restrict__ scores,
                        const int64_t* __restrict__ labels, const int32_t* __restrict__ pass_idx, int64_t m, int npass, int C,
                        AugArgs a, float* __restrict__ boxes_out, float* __restrict__ boxes_nms, float* __restrict__ scores_t) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (int64_t)gridDim.x * blockDim.x) {
    const float* b = boxes + i * box_stride;
    float v[16];
    for (int c = 0; c < D; ++c) v[c] = b[c];
    const int k = pass_idx[i];
    const bool ok = k >= 0 && k < npass;
    if (ok) {
      const AugDesc& d = a.d[k];
      const bool vel = D >= 9;
      if (d.flip_v) {
        v[0] = -v[0];
        if (vel) v[7] = -v[7];
        v[6] = -v[6];
      }
      if (d.flip_h) {
        v[1] = -v[1];
        if (vel) v[8] = -v[8];
        v[6] = __fadd_rn(-v[6], AUG_PI);
      }
      for (int c = 0; c < 6; ++c) v[c] = __fmul_rn(v[c], d.scale);  // (d.scale holds fp32(1 / s) here)
      for (int c = 7; c < D; ++c) v[c] = __fmul_rn(v[c], d.scale);
      if (d.rot) {
        const float x = __fadd_rn(__fmul_rn(v[0], d.c), __fmul_rn(v[1], d.s));
        const float y = __fsub_rn(__fmul_rn(v[1], d.c), __fmul_rn(v[0], d.s));
        v[0] = x;
        v[1] = y;
        if (vel) {
          const float vx = __fadd_rn(__fmul_rn(v[7], d.c), __fmul_rn(v[8], d.s));
          const float vy = __fsub_rn(__fmul_rn(v[8], d.c), __fmul_rn(v[7], d.s));
          v[7] = vx;
          v[8] = vy;
        }
        v[6] = __fadd_rn(v[6], d.theta);
      }
    }
    float* o = boxes_out + i * D;
    for (int c = 0; c < D; ++c) o[c] = v[c];
    const float hw = __fmul_rn(v[3], 0.5f), hh = __fmul_rn(v[4], 0.5f);  // xywhr2xyxyr(boxes.bev)
    float* q = boxes_nms + i * 5;
    q[0] = __fsub_rn(v[0], hw); q[1] = __fsub_rn(v[1], hh); q[2] = __fadd_rn(v[0], hw); q[3] = __fadd_rn(v[1], hh); q[4] = v[6];
    const int64_t lab = labels[i];
    const float s = scores[i];
    for (int c = 0; c < C; ++c) scores_t[(int64_t)c * m + i] = (ok && lab == c) ? s : -INFINITY;  // (-inf: never above a threshold)
  }
}

static int aug_fill_descs(AugArgs& a, const float* desc, int32_t n) {
  if (n < 1 || n > AUG_MAX || !desc) return FSF_ERR_INVALID_ARG;
  for (int k = 0; k < n; ++k) {
    const float* d = desc + 7 * k;
    a.d[k].c = d[0]; a.d[k].s = d[1]; a.d[k].scale = d[2]; a.d[k].theta = d[3];
    a.d[k].rot = d[4] != 0.0f; a.d[k].flip_h = d[5] != 0.0f; a.d[k].flip_v = d[6] != 0.0f;
    if (!(d[2] > 0.0f)) return FSF_ERR_INVALID_ARG;
  }
  a.naug = n;
  return FSF_OK;
}

}  // namespace fsf

using namespace fsf;

extern "C" int32_t fsf_augment_max(void) { return AUG_MAX; }

struct AugLayout {
  uint32_t* tile_sums;
  int64_t* tot;
  AugArgs* a_dev;
  AugLayout(FsfArena& arena, int64_t total)
      : tile_sums(arena.take<uint32_t>(scan_num_tiles(total))), tot(arena.take<int64_t>(1)), a_dev(arena.take<AugArgs>(1)) {}
};

extern "C" int64_t fsf_augment_points_workspace_bytes(int64_t n_rows, int32_t num_augs) {
  if (n_rows < 0 || num_augs < 1) return 0;
  return fsf_layout_bytes<AugLayout>(n_rows * num_augs);
}

extern "C" int fsf_augment_points(const float* points, int64_t n_rows, int32_t cols, const float* aug_desc, int32_t num_augs,
                                  const float* pc_range, float* out, int64_t* offsets_dev, int64_t* offsets_host, void* workspace,
                                  int64_t workspace_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (n_rows < 0 || cols < 3 || cols > 64 || (n_rows > 0 && (!points || !out)) || !offsets_dev) return FSF_ERR_INVALID_ARG;
  if (n_rows * (int64_t)num_augs >= ((int64_t)1 << 31)) return FSF_ERR_UNSUPPORTED;
  AugArgs a;
  const int rc0 = aug_fill_descs(a, aug_desc, num_augs);
  if (rc0 != FSF_OK) return rc0;
  const int64_t total = n_rows * num_augs;
  FSF_CARVE(AugLayout, l, workspace, workspace_bytes, total);
  a.in = points; a.out = out; a.offsets = offsets_dev; a.n = n_rows; a.cols = cols;
  a.use_range = pc_range ? 1 : 0;
  for (int k = 0; k < 6; ++k) a.range[k] = pc_range ? pc_range[k] : 0.0f;
  FSF_HIP_TRY(hipMemsetAsync(offsets_dev, 0, sizeof(int64_t) * (num_augs + 1), stream));
  FSF_HIP_TRY(hipMemcpyAsync(l.a_dev, &a, sizeof(AugArgs), hipMemcpyHostToDevice, stream));  // (pageable source: staged before return)
  if (total > 0) {
    const int rc = exclusive_scan_u32(AugIn{l.a_dev}, AugOut{l.a_dev}, total, l.tile_sums, nullptr, l.tot, stream);
    if (rc != FSF_OK) return rc;
  }
  if (offsets_host) {
    FSF_READ_BACK(offsets_host, offsets_dev, sizeof(int64_t) * (num_augs + 1), stream);
  }
  return FSF_OK;
}

extern "C" int fsf_aug_boxes_map_back(const float* boxes, int64_t box_stride, int32_t box_dim, const float* scores,
                                      const int64_t* labels, const int32_t* pass_idx, int64_t m, const float* pass_desc,
                                      int32_t num_passes, int32_t num_classes, float* boxes_out, float* boxes_nms, float* scores_t,
                                      void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (m < 0 || box_dim < 7 || box_dim > 16 || box_stride < box_dim || num_classes < 1 ||
      (m > 0 && (!boxes || !scores || !labels || !pass_idx || !boxes_out || !boxes_nms || !scores_t)))
    return FSF_ERR_INVALID_ARG;
  AugArgs a;
  const int rc0 = aug_fill_descs(a, pass_desc, num_passes);
  if (rc0 != FSF_OK) return rc0;
  a.in = nullptr; a.out = nullptr; a.offsets = nullptr; a.n = 0; a.cols = 0; a.use_range = 0;
  for (int k = 0; k < 6; ++k) a.range[k] = 0.0f;
  if (m == 0) return FSF_OK;
  hipLaunchKernelGGL(aug_map_back_kernel, dim3(fsf_stream_grid(m, 256)), dim3(256), 0, stream, boxes, box_stride, (int)box_dim, scores,
                     labels, pass_idx, m, (int)num_passes, (int)num_classes, a, boxes_out, boxes_nms, scores_t);
  FSF_LAUNCH_CHECK();
  return FSF_OK;
}
