// K40: train-time augmentation on the device — see include/fsf_hip.h and docs/kernels/K40_train_augment.md.
//   fsf_train_augment_points (K40a + radix sort + K40b): one uploaded cloud -> the flipped, rotated, scaled, translated, range-filtered
//                                   and shuffled cloud of the train pipeline.  K40a transforms each row's xyz, tests the range and writes
//                                   the pair (key, row), key = dropped << 31 | mix31(row, seed), plus the survivor count; the stable radix
//                                   sort of the n_rows pairs puts the survivors first in key order (= the shuffle); K40b gathers row
//                                   vals[j] into output row j and transforms its xyz AGAIN: the row is read whole for its feature columns
//                                   anyway, so the second transform costs ~20 VALU operations and no traffic, where staging the xyz would
//                                   cost 12 B written and 12 B read per row.
//   fsf_train_augment_boxes  (K40c): the GT boxes of a whole batch in one launch: flips, rotation, scale, translation, the BEV range
//                                   mask of MyObjectRangeFilter as label -1, limit_yaw; the same mask and wrap on the no-aug boxes.
// Arithmetic is pinned: every product, sum and quotient is rounded on its own (__fmul_rn / __fadd_rn / __fsub_rn /
// __fdiv_rn, no FMA contraction), in the order of datasets/train_augment.py::augment_points_host / augment_boxes_host.
#include "common.h"
#include "radix_sort.h"

namespace fsf {

constexpr float TA_PI = 3.14159265358979323846f;      // np.pi as an fp32 scalar operand
constexpr float TA_TWO_PI = 6.28318530717958647692f;  // fp32(2 * np.pi), limit_yaw's period

struct TaDesc {
  float c, s, scale, theta;  // cos / sin of the fp32 angle (host torch.cos / torch.sin), scale, the angle itself (the boxes' yaw)
  float t[3];                // translation, each component rounded to fp32
  int rot, flip_h, flip_v;   // rot = 0: the angle is exactly zero and the rotation is not evaluated
};

struct TaPointArgs {
  TaDesc d;
  float range[6];
  int use_range, shuffle;
  uint32_t seed_lo, seed_hi;
};

struct TaBoxArgs {
  int nb;
  int64_t off[FSF_TRAIN_AUGMENT_MAX_BATCH + 1];
  TaDesc d[FSF_TRAIN_AUGMENT_MAX_BATCH];
  float range[4];  // x min, y min, x max, y max
};

static void ta_fill_desc(TaDesc& d, const float* v) {
  d.c = v[0]; d.s = v[1]; d.scale = v[2]; d.theta = v[3];
  d.rot = v[4] != 0.0f; d.flip_h = v[5] != 0.0f; d.flip_v = v[6] != 0.0f;
  d.t[0] = v[7]; d.t[1] = v[8]; d.t[2] = v[9];
}

// the key mix (docs/kernels/K40_train_augment.md, "Key mix"): murmur3's 32-bit finaliser over the row index and the seed's two halves,
// shifted to 31 bits — datasets/train_augment.py::shuffle_keys_host is the same integer arithmetic
__device__ __forceinline__ uint32_t ta_mix31(uint32_t row, uint32_t seed_lo, uint32_t seed_hi) {
  uint32_t h = (row ^ seed_lo) + seed_hi * 0x9E3779B9u;
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  h *= 0xC2B2AE35u;
  h ^= h >> 16;
  return h >> 1;
}

__device__ __forceinline__ void ta_rotate(const TaDesc& d, float& x, float& y) {
  const float xr = __fsub_rn(__fmul_rn(x, d.c), __fmul_rn(y, d.s));
  const float yr = __fadd_rn(__fmul_rn(x, d.s), __fmul_rn(y, d.c));
  x = xr;
  y = yr;
}

// train pipeline order: horizontal then vertical flip (RandomFlip3D), rotation, scale, translation (GlobalRotScaleTrans), then the strict
// in-range test (PointsRangeFilter); a NaN coordinate fails every comparison and the row is dropped
__device__ __forceinline__ bool ta_point(const TaPointArgs& a, float& x, float& y, float& z) {
  const TaDesc& d = a.d;
  if (d.flip_h) y = -y;
  if (d.flip_v) x = -x;
  if (d.rot) ta_rotate(d, x, y);
  x = __fadd_rn(__fmul_rn(x, d.scale), d.t[0]);
  y = __fadd_rn(__fmul_rn(y, d.scale), d.t[1]);
  z = __fadd_rn(__fmul_rn(z, d.scale), d.t[2]);
  if (!a.use_range) return true;
  return x > a.range[0] && y > a.range[1] && z > a.range[2] && x < a.range[3] && y < a.range[4] && z < a.range[5];
}

// K40a
__global__ void __launch_bounds__(256)
    train_aug_keys_kernel(const float* __restrict__ in, int64_t n, int cols, TaPointArgs a, uint64_t* __restrict__ keys,
                          uint32_t* __restrict__ vals, unsigned long long* __restrict__ count) {
  __shared__ uint32_t wave_kept[4];
  uint32_t kept = 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const float* p = in + i * cols;
    float x = p[0], y = p[1], z = p[2];
    const bool keep = ta_point(a, x, y, z);
    // without the shuffle one key bit is enough: the stable sort of it is the stable compaction in source order
    const uint32_t key = a.shuffle ? ((keep ? 0u : 0x80000000u) | ta_mix31((uint32_t)i, a.seed_lo, a.seed_hi)) : (keep ? 0u : 1u);
    keys[i] = key;
    vals[i] = (uint32_t)i;
    kept += keep ? 1u : 0u;
  }
  kept = fsf_wave_sum(kept);
  if (fsf_lane() == 0) wave_kept[threadIdx.x >> 6] = kept;
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t block_kept = wave_kept[0] + wave_kept[1] + wave_kept[2] + wave_kept[3];
    if (block_kept) atomicAdd(count, (unsigned long long)block_kept);  // (integer: the sum does not depend on the order)
  }
}

// K40b: output row j < count = the transformed source row vals[j]; VEC: cols % 4 == 0 and both tensors 16-byte aligned
template <bool VEC>
__global__ void __launch_bounds__(256)
    train_aug_gather_kernel(const float* __restrict__ in, int64_t n, int cols, TaPointArgs a, const uint32_t* __restrict__ vals,
                            const int64_t* __restrict__ count, float* __restrict__ out) {
  int64_t m = *count;
  if (m > n) m = n;
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < m; j += (int64_t)gridDim.x * blockDim.x) {
    const int64_t src = vals[j];
    if (src >= n) continue;  // (cannot happen: the sort permutes [0, n))
    const float* p = in + src * cols;
    float* o = out + j * cols;
    if (VEC) {
      float4 v = *reinterpret_cast<const float4*>(p);
      ta_point(a, v.x, v.y, v.z);
      *reinterpret_cast<float4*>(o) = v;
      for (int c = 4; c < cols; c += 4) *reinterpret_cast<float4*>(o + c) = *reinterpret_cast<const float4*>(p + c);
    } else {
      float x = p[0], y = p[1], z = p[2];
      ta_point(a, x, y, z);
      o[0] = x; o[1] = y; o[2] = z;
      for (int c = 3; c < cols; ++c) o[c] = p[c];  // features and the no-aug xyz (SaveNoAugPoints) unchanged
    }
  }
}

// limit_yaw(offset = 0.5, period = 2 pi): v - floor(v / period + 0.5) * period, every step an fp32 operation
__device__ __forceinline__ float ta_limit_yaw(float v) {
  const float k = floorf(__fadd_rn(__fdiv_rn(v, TA_TWO_PI), 0.5f));
  return __fsub_rn(v, __fmul_rn(k, TA_TWO_PI));
}

// K40c: one thread per box
__global__ void __launch_bounds__(256)
    train_aug_boxes_kernel(const float* __restrict__ boxes, int64_t box_stride, const int64_t* __restrict__ labels,
                           const float* __restrict__ na_boxes, int64_t na_stride, const int64_t* __restrict__ na_labels, int64_t g, int D,
                           TaBoxArgs a, float* __restrict__ boxes_out, int64_t* __restrict__ labels_out, float* __restrict__ na_boxes_out,
                           int64_t* __restrict__ na_labels_out) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < g; i += (int64_t)gridDim.x * blockDim.x) {
    int k = 0;
    while (k + 1 < a.nb && i >= a.off[k + 1]) ++k;  // the box's sample (nb <= 32)
    const TaDesc& d = a.d[k];
    const float* b = boxes + i * box_stride;
    float v[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) v[c] = c < D ? b[c] : 0.0f;
    const bool vel = D >= 9;
    if (d.flip_h) {
      v[1] = -v[1];
      if (vel) v[8] = -v[8];
      v[6] = __fadd_rn(-v[6], TA_PI);
    }
    if (d.flip_v) {
      v[0] = -v[0];
      if (vel) v[7] = -v[7];
      v[6] = -v[6];
    }
    if (d.rot) {
      ta_rotate(d, v[0], v[1]);
      if (vel) ta_rotate(d, v[7], v[8]);
      v[6] = __fadd_rn(v[6], d.theta);  // (box_contain.h's frame, the one every GT consumer tests: the footprint turns with the scene)
    }
#pragma unroll
    for (int c = 0; c < 16; ++c)
      if (c != 6) v[c] = __fmul_rn(v[c], d.scale);
    v[0] = __fadd_rn(v[0], d.t[0]);
    v[1] = __fadd_rn(v[1], d.t[1]);
    v[2] = __fadd_rn(v[2], d.t[2]);
    const bool keep = v[0] > a.range[0] && v[1] > a.range[1] && v[0] < a.range[2] && v[1] < a.range[3];  // in_range_bev, strict
    v[6] = ta_limit_yaw(v[6]);
    float* o = boxes_out + i * D;
#pragma unroll
    for (int c = 0; c < 16; ++c)
      if (c < D) o[c] = v[c];
    const float* nb = na_boxes + i * na_stride;
    float* no = na_boxes_out + i * D;
#pragma unroll
    for (int c = 0; c < 16; ++c)
      if (c < D) no[c] = c == 6 ? ta_limit_yaw(nb[c]) : nb[c];
    const int64_t lab = labels[i], na_lab = na_labels[i];
    labels_out[i] = (keep || lab < 0) ? lab : -1;
    na_labels_out[i] = (keep || na_lab < 0) ? na_lab : -1;
  }
}

}  // namespace fsf

using namespace fsf;

extern "C" int64_t fsf_train_augment_points_workspace_bytes(int64_t n_rows) {
  if (n_rows < 0) return 0;
  return radix_sort_scratch_bytes(n_rows);
}

extern "C" int fsf_train_augment_points(const float* points, int64_t n_rows, int32_t cols, const float* desc, const float* pc_range,
                                        int64_t shuffle_seed, float* out, int64_t* count_dev, int64_t* count_host, void* workspace,
                                        int64_t workspace_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (n_rows < 0 || cols < 3 || cols > 64 || (n_rows > 0 && (!points || !out)) || !count_dev || !desc) return FSF_ERR_INVALID_ARG;
  if (n_rows >= ((int64_t)1 << 31)) return FSF_ERR_UNSUPPORTED;
  if (!(desc[2] > 0.0f)) return FSF_ERR_INVALID_ARG;
  FSF_CARVE(RadixScratch, s, workspace, workspace_bytes, n_rows);  // (the sort's scratch is all this entry takes: the query is radix_sort_scratch_bytes)
  TaPointArgs a;
  ta_fill_desc(a.d, desc);
  a.use_range = pc_range ? 1 : 0;
  for (int k = 0; k < 6; ++k) a.range[k] = pc_range ? pc_range[k] : 0.0f;
  a.shuffle = shuffle_seed >= 0 ? 1 : 0;
  a.seed_lo = (uint32_t)((uint64_t)shuffle_seed & 0xFFFFFFFFu);
  a.seed_hi = (uint32_t)((uint64_t)shuffle_seed >> 32);
  FSF_HIP_TRY(hipMemsetAsync(count_dev, 0, sizeof(int64_t), stream));
  if (n_rows > 0) {
    const int grid = fsf_stream_grid(n_rows, 256);
    hipLaunchKernelGGL(train_aug_keys_kernel, dim3(grid), dim3(256), 0, stream, points, n_rows, (int)cols, a, s.keys_a, s.vals_a,
                       reinterpret_cast<unsigned long long*>(count_dev));
    FSF_LAUNCH_CHECK();
    uint64_t* keys_sorted = nullptr;
    uint32_t* vals_sorted = nullptr;
    const int rc = radix_sort_pairs(s.keys_a, s.vals_a, s.keys_b, s.vals_b, s.hist, n_rows, a.shuffle ? 32 : 1, &keys_sorted, &vals_sorted, stream);
    if (rc != FSF_OK) return rc;
    const bool vec = cols % 4 == 0 && ((uintptr_t)points % 16) == 0 && ((uintptr_t)out % 16) == 0;
    if (vec)
      hipLaunchKernelGGL(train_aug_gather_kernel<true>, dim3(grid), dim3(256), 0, stream, points, n_rows, (int)cols, a, vals_sorted,
                         count_dev, out);
    else
      hipLaunchKernelGGL(train_aug_gather_kernel<false>, dim3(grid), dim3(256), 0, stream, points, n_rows, (int)cols, a, vals_sorted,
                         count_dev, out);
    FSF_LAUNCH_CHECK();
  }
  if (count_host) {
    FSF_READ_BACK(count_host, count_dev, sizeof(int64_t), stream);
  }
  return FSF_OK;
}

extern "C" int fsf_train_augment_boxes(const float* boxes, int64_t box_stride, int32_t box_dim, const int64_t* labels,
                                       const float* no_aug_boxes, int64_t no_aug_stride, const int64_t* no_aug_labels,
                                       const int64_t* sample_offsets, int32_t num_samples, const float* desc, const float* pc_range,
                                       float* boxes_out, int64_t* labels_out, float* no_aug_boxes_out, int64_t* no_aug_labels_out,
                                       void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (num_samples < 1 || num_samples > FSF_TRAIN_AUGMENT_MAX_BATCH || !sample_offsets || !desc || !pc_range || box_dim < 7 ||
      box_dim > 16 || box_stride < box_dim || no_aug_stride < box_dim || sample_offsets[0] != 0)
    return FSF_ERR_INVALID_ARG;
  TaBoxArgs a;
  a.nb = num_samples;
  for (int k = 0; k < num_samples; ++k) {
    if (sample_offsets[k + 1] < sample_offsets[k] || !(desc[10 * k + 2] > 0.0f)) return FSF_ERR_INVALID_ARG;
    ta_fill_desc(a.d[k], desc + 10 * k);
  }
  for (int k = 0; k <= FSF_TRAIN_AUGMENT_MAX_BATCH; ++k) a.off[k] = sample_offsets[k <= num_samples ? k : num_samples];
  a.range[0] = pc_range[0]; a.range[1] = pc_range[1]; a.range[2] = pc_range[3]; a.range[3] = pc_range[4];
  const int64_t g = sample_offsets[num_samples];
  if (g == 0) return FSF_OK;
  if (g >= ((int64_t)1 << 31)) return FSF_ERR_UNSUPPORTED;
  if (!boxes || !labels || !no_aug_boxes || !no_aug_labels || !boxes_out || !labels_out || !no_aug_boxes_out || !no_aug_labels_out)
    return FSF_ERR_INVALID_ARG;
  hipLaunchKernelGGL(train_aug_boxes_kernel, dim3(fsf_stream_grid(g, 256)), dim3(256), 0, stream, boxes, box_stride, labels, no_aug_boxes,
                     no_aug_stride, no_aug_labels, g, (int)box_dim, a, boxes_out, labels_out, no_aug_boxes_out, no_aug_labels_out);
  FSF_LAUNCH_CHECK();
  return FSF_OK;
}
