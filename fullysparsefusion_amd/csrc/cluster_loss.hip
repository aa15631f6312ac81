// K36: the query heads' training targets and losses — see include/fsf_hip.h and docs/kernels/K36_cluster_losses.md.
//   fsf_cluster_targets        (K36a): cluster centres + per-sample GT boxes (already regrouped for the task) -> int64 labels, encoded
//                                      box targets, box weights, assigned box index, log scalars and the two averaging factors.
//                                      Three launches: per-box constants (one lane per box), one lane per cluster looping over its
//                                      sample's boxes (first hit wins, K35a's test), then one workgroup for the counts.
//   fsf_cluster_loss_forward   (K36b): sigmoid focal loss over every (row, class) / cls_avg_factor, and the L1 groups centre / size /
//                                      rotation (/ reg_avg_factor) and velocity (mean) over the positive rows.  Knows nothing about
//                                      boxes: any assigner that produces labels, targets and weights can feed it.  One lane per row,
//                                      fp64 terms and per-workgroup partials, one final workgroup in fixed order.
//   fsf_cluster_loss_backward  (K36c): dense grad_cls_logits / grad_reg_preds; the sigmoid is recomputed.  One lane per output element.
// No float atomics and no host synchronisation: the same inputs give bit-identical outputs from run to run.
#include "box_contain.h"
#include "cluster_encode.h"
#include "common.h"

namespace fsf {

constexpr int CL_BLOCK = 256;
constexpr int CL_NUM_LOSSES = 5;  // cls, center, size, rot, vel
constexpr int CL_PARTS = CL_NUM_LOSSES + 1;  // + the number of positive rows

struct ClusterLossWeights {
  float gamma, alpha, cls, center, size, rot, vel;
};

// ------------------------------------------------------------------------------------------------ K36a
// Per box: K35a's containment constants of the box enlarged by e (dims + 2e, z_bottom - e; e = 0 leaves every value as it is), the
// coder's encoded values (cluster_encode.h), and the box's hit flag cleared.
__global__ void __launch_bounds__(CL_BLOCK) cluster_box_prep_kernel(const float* __restrict__ boxes, int64_t num_boxes, int64_t box_stride,
                                                                    float enlarge, float* __restrict__ table, float* __restrict__ enc,
                                                                    int32_t* __restrict__ box_hit) {
  const int64_t k = (int64_t)blockIdx.x * CL_BLOCK + threadIdx.x;
  if (k >= num_boxes) return;
  const float* b = boxes + k * box_stride;
  const float e2 = __fmul_rn(enlarge, 2.0f);
  box_constants(b[0], b[1], __fsub_rn(b[2], enlarge), __fadd_rn(b[3], e2), __fadd_rn(b[4], e2), __fadd_rn(b[5], e2), b[6],
                table + k * BOX_WORDS);
  cluster_encode_box(b, enc + k * CL_ENC_WORDS);
  box_hit[k] = 0;
}

template <typename BT>
__global__ void __launch_bounds__(CL_BLOCK) cluster_targets_kernel(const float* __restrict__ xyz, int64_t n, int64_t xyz_stride,
                                                                   const BT* __restrict__ batch_idx, int64_t batch_stride,
                                                                   const int32_t* __restrict__ box_ptr, int32_t num_samples,
                                                                   const float* __restrict__ boxes, int64_t box_stride, int32_t box_cols,
                                                                   const float* __restrict__ table, const float* __restrict__ enc,
                                                                   const int32_t* __restrict__ box_labels, int32_t num_classes,
                                                                   int32_t code_size, int64_t* __restrict__ labels,
                                                                   float* __restrict__ bbox_targets, float* __restrict__ bbox_weights,
                                                                   int32_t* __restrict__ assigned, int32_t* __restrict__ box_hit,
                                                                   int32_t* __restrict__ partial_count) {
  const int64_t i = (int64_t)blockIdx.x * CL_BLOCK + threadIdx.x;
  int hit_count = 0;
  if (i < n) {
    const float* p = xyz + i * xyz_stride;
    const float q[3] = {p[0], p[1], p[2]};
    const int64_t b = (int64_t)batch_idx[i * batch_stride];
    int k0 = 0;
    int hit = -1;
    if (b >= 0 && b < num_samples) {
      k0 = box_ptr[b];
      hit = first_box_containing(q[0], q[1], q[2], table, box_labels, k0, box_ptr[b + 1]);
    }
    hit_count = cluster_write_target_rows(i, q, hit, boxes, box_stride, box_cols, enc, box_labels, num_classes, code_size, labels,
                                          bbox_targets, bbox_weights, box_hit);
    assigned[i] = hit >= 0 ? hit - k0 : -1;
  }
  cluster_block_count<CL_BLOCK>(hit_count, partial_count);
}

__global__ void __launch_bounds__(CL_BLOCK) cluster_targets_final_kernel(const int32_t* __restrict__ partial, int64_t num_partials,
                                                                         const int32_t* __restrict__ box_labels,
                                                                         const int32_t* __restrict__ box_hit, int64_t num_boxes, int64_t n,
                                                                         bool hits_valid, float* __restrict__ stats) {
  cluster_stats_final<CL_BLOCK>(partial, num_partials, box_labels, box_hit, num_boxes, n, hits_valid, stats);
}

// ------------------------------------------------------------------------------------------------ K36b / K36c shared
// softplus(x) = log(1 + exp(x)) without overflow and without log(0): log p = -softplus(-z), log(1 - p) = -softplus(z).
__device__ __forceinline__ double softplus64(double x) { return fmax(x, 0.0) + log1p(exp(-fabs(x))); }

__device__ __forceinline__ bool label_is_positive(int64_t y, int32_t num_classes) { return y >= 0 && y < num_classes; }

// L1 group of a regression column: 0 centre, 1 size, 2 rotation, 3 velocity.
__device__ __forceinline__ int reg_group(int c) { return c < 3 ? 0 : (c < 6 ? 1 : (c < 8 ? 2 : 3)); }

// ------------------------------------------------------------------------------------------------ K36b
// partials[block] = (sum of focal terms, sums of |pred - target| * weight of the four groups over the positive rows, positive rows).
__global__ void __launch_bounds__(CL_BLOCK) cluster_loss_partials_kernel(const float* __restrict__ cls_logits, int64_t ld_cls,
                                                                         const float* __restrict__ reg_preds, int64_t ld_reg, int64_t n,
                                                                         int32_t num_classes, int32_t code_size,
                                                                         const int64_t* __restrict__ labels,
                                                                         const float* __restrict__ label_weights,
                                                                         const float* __restrict__ bbox_targets,
                                                                         const float* __restrict__ bbox_weights, float gamma, float alpha,
                                                                         double* __restrict__ partials) {
  __shared__ double wave_part[CL_PARTS][CL_BLOCK / FSF_WAVE];
  const int64_t i = (int64_t)blockIdx.x * CL_BLOCK + threadIdx.x;
  double acc[CL_PARTS];
#pragma unroll
  for (int q = 0; q < CL_PARTS; ++q) acc[q] = 0.0;
  if (i < n) {
    const int64_t y = labels[i];
    const float* z = cls_logits + i * ld_cls;
    const double g = (double)gamma, a = (double)alpha;
    double fl = 0.0;
    for (int c = 0; c < num_classes; ++c) {
      const double zc = (double)z[c];
      const double sp_pos = softplus64(zc), sp_neg = softplus64(-zc);  // -log(1 - p), -log p
      fl += (c == y) ? a * exp(-g * sp_pos) * sp_neg : (1.0 - a) * exp(-g * sp_neg) * sp_pos;
    }
    acc[0] = label_weights ? fl * (double)label_weights[i] : fl;
    if (label_is_positive(y, num_classes)) {
      const float* r = reg_preds + i * ld_reg;
      const float* t = bbox_targets + i * code_size;
      const float* w = bbox_weights + i * code_size;
      for (int c = 0; c < code_size; ++c) acc[1 + reg_group(c)] += fabs((double)r[c] - (double)t[c]) * (double)w[c];
      acc[5] = 1.0;
    }
  }
#pragma unroll
  for (int q = 0; q < CL_PARTS; ++q) {
    const double s = fsf_wave_sum(acc[q]);
    if (fsf_lane() == 0) wave_part[q][threadIdx.x / FSF_WAVE] = s;
  }
  __syncthreads();
  if (threadIdx.x < CL_PARTS) {
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < CL_BLOCK / FSF_WAVE; ++w) s += wave_part[threadIdx.x][w];
    partials[(int64_t)blockIdx.x * CL_PARTS + threadIdx.x] = s;
  }
}

__global__ void __launch_bounds__(CL_BLOCK) cluster_loss_final_kernel(const double* __restrict__ partials, int64_t num_partials,
                                                                      const float* __restrict__ avg_factors, ClusterLossWeights lw,
                                                                      bool with_vel, float* __restrict__ losses, int64_t* __restrict__ counts) {
  __shared__ double wave_part[CL_PARTS][CL_BLOCK / FSF_WAVE];
  double acc[CL_PARTS];
#pragma unroll
  for (int q = 0; q < CL_PARTS; ++q) acc[q] = 0.0;
  for (int64_t j = threadIdx.x; j < num_partials; j += CL_BLOCK) {
#pragma unroll
    for (int q = 0; q < CL_PARTS; ++q) acc[q] += partials[j * CL_PARTS + q];
  }
#pragma unroll
  for (int q = 0; q < CL_PARTS; ++q) {
    const double s = fsf_wave_sum(acc[q]);
    if (fsf_lane() == 0) wave_part[q][threadIdx.x / FSF_WAVE] = s;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double t[CL_PARTS];
#pragma unroll
    for (int q = 0; q < CL_PARTS; ++q) {
      t[q] = 0.0;
#pragma unroll
      for (int w = 0; w < CL_BLOCK / FSF_WAVE; ++w) t[q] += wave_part[q][w];
    }
    const int64_t num_pos = (int64_t)t[5];
    const double cls_avg = (double)avg_factors[0], reg_avg = (double)avg_factors[1];
    losses[0] = (float)((double)lw.cls * (t[0] / cls_avg));
    losses[1] = num_pos > 0 ? (float)((double)lw.center * (t[1] / reg_avg)) : 0.f;
    losses[2] = num_pos > 0 ? (float)((double)lw.size * (t[2] / reg_avg)) : 0.f;
    losses[3] = num_pos > 0 ? (float)((double)lw.rot * (t[3] / reg_avg)) : 0.f;
    losses[4] = (with_vel && num_pos > 0) ? (float)((double)lw.vel * (t[4] / (2.0 * (double)num_pos))) : 0.f;
    counts[0] = num_pos;
  }
}

// ------------------------------------------------------------------------------------------------ K36c
// grad_cls[i, c] = dFL/dz * label_weight_i * w_cls * g_cls / cls_avg_factor, with p = sigmoid(z), q = 1 - p:
//   c == y:  alpha q^gamma (gamma p log p - q)            else:  (1 - alpha) p^gamma (p - gamma q log q)
// grad_reg[i, c] = sign(pred - target) * weight * w_group * g_group / (reg_avg_factor | 2 num_pos) on positive rows, else 0.
__global__ void __launch_bounds__(CL_BLOCK) cluster_loss_backward_kernel(const float* __restrict__ cls_logits, int64_t ld_cls,
                                                                         const float* __restrict__ reg_preds, int64_t ld_reg, int64_t n,
                                                                         int32_t num_classes, int32_t code_size,
                                                                         const int64_t* __restrict__ labels,
                                                                         const float* __restrict__ label_weights,
                                                                         const float* __restrict__ bbox_targets,
                                                                         const float* __restrict__ bbox_weights,
                                                                         const float* __restrict__ avg_factors, ClusterLossWeights lw,
                                                                         bool with_vel, const int64_t* __restrict__ counts,
                                                                         const float* __restrict__ g_cls, const float* __restrict__ g_center,
                                                                         const float* __restrict__ g_size, const float* __restrict__ g_rot,
                                                                         const float* __restrict__ g_vel, float* __restrict__ grad_cls,
                                                                         float* __restrict__ grad_reg) {
  const int64_t n_cls = n * num_classes, n_all = n_cls + n * code_size;
  const int64_t num_pos = counts[0];
  const double cls_avg = (double)avg_factors[0], reg_avg = (double)avg_factors[1];
  const double cls_scale = g_cls ? (double)lw.cls * (double)g_cls[0] / cls_avg : 0.0;
  double reg_scale[4] = {0.0, 0.0, 0.0, 0.0};
  if (num_pos > 0) {
    if (g_center) reg_scale[0] = (double)lw.center * (double)g_center[0] / reg_avg;
    if (g_size) reg_scale[1] = (double)lw.size * (double)g_size[0] / reg_avg;
    if (g_rot) reg_scale[2] = (double)lw.rot * (double)g_rot[0] / reg_avg;
    if (g_vel && with_vel) reg_scale[3] = (double)lw.vel * (double)g_vel[0] / (2.0 * (double)num_pos);
  }
  const double g = (double)lw.gamma, a = (double)lw.alpha;
  for (int64_t e = (int64_t)blockIdx.x * CL_BLOCK + threadIdx.x; e < n_all; e += (int64_t)gridDim.x * CL_BLOCK) {
    if (e < n_cls) {
      const int64_t i = e / num_classes;
      const int c = (int)(e - i * num_classes);
      const double zc = (double)cls_logits[i * ld_cls + c];
      const double sp_pos = softplus64(zc), sp_neg = softplus64(-zc);  // -log q, -log p
      const double p = exp(-sp_neg), q = exp(-sp_pos);
      const double d = (c == labels[i]) ? a * exp(-g * sp_pos) * (-g * p * sp_neg - q) : (1.0 - a) * exp(-g * sp_neg) * (p + g * q * sp_pos);
      const double s = label_weights ? cls_scale * (double)label_weights[i] : cls_scale;
      grad_cls[e] = (float)(d * s);
    } else {
      const int64_t r = e - n_cls;
      const int64_t i = r / code_size;
      const int c = (int)(r - i * code_size);
      float out = 0.f;
      if (label_is_positive(labels[i], num_classes)) {
        const double d = (double)reg_preds[i * ld_reg + c] - (double)bbox_targets[r];
        const double s = reg_scale[reg_group(c)] * (double)bbox_weights[r];
        out = (float)(d > 0.0 ? s : (d < 0.0 ? -s : 0.0));
      }
      grad_reg[r] = out;
    }
  }
}

static int cluster_loss_check(const float* cls_logits, int64_t ld_cls, const float* reg_preds, int64_t ld_reg, int64_t n,
                              int32_t num_classes, int32_t code_size, const int64_t* labels, const float* bbox_targets,
                              const float* bbox_weights, const float* avg_factors) {
  if (n < 0 || num_classes < 1 || (code_size != 8 && code_size != 10) || ld_cls < num_classes || ld_reg < code_size) return FSF_ERR_INVALID_ARG;
  if (!avg_factors || (n > 0 && (!cls_logits || !reg_preds || !labels || !bbox_targets || !bbox_weights))) return FSF_ERR_INVALID_ARG;
  if (n >= ((int64_t)1 << 40) || n * ((int64_t)num_classes + code_size) >= ((int64_t)1 << 46)) return FSF_ERR_UNSUPPORTED;
  return FSF_OK;
}

}  // namespace fsf

using namespace fsf;

struct ClTargetsLayout {
  int nblk;
  float *table, *enc;
  int32_t *box_hit, *partial;
  ClTargetsLayout(FsfArena& arena, int64_t num_boxes, int64_t n)
      : nblk(fsf_cdiv(n, CL_BLOCK)), table(arena.take<float>(BOX_WORDS * num_boxes)), enc(arena.take<float>(CL_ENC_WORDS * num_boxes)),
        box_hit(arena.take<int32_t>(num_boxes)), partial(arena.take<int32_t>(nblk)) {}
};
// (one slice: a function in place of a layout struct, taken from a hand-made arena in the entry)
static double* cluster_loss_layout(FsfArena& arena, int64_t n) { return arena.take<double>(CL_PARTS * (int64_t)fsf_cdiv(n, CL_BLOCK)); }

extern "C" int64_t fsf_cluster_targets_workspace_bytes(int64_t num_boxes, int64_t n) {
  if (num_boxes < 0 || n < 0) return -1;
  return fsf_layout_bytes<ClTargetsLayout>(num_boxes, n);
}

extern "C" int fsf_cluster_targets(const float* cluster_xyz, int64_t n, int64_t xyz_stride, const void* batch_idx, int32_t batch_idx_bytes,
                                   int64_t batch_stride, const int32_t* box_ptr, int32_t num_samples, const float* boxes,
                                   int64_t num_boxes, int64_t box_stride, int32_t box_cols, const int32_t* box_labels,
                                   int32_t num_classes, int32_t code_size, float enlarge_width, void* workspace, int64_t workspace_bytes,
                                   int64_t* labels, float* bbox_targets, float* bbox_weights, int32_t* assigned, float* stats,
                                   void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (n < 0 || num_samples < 0 || num_boxes < 0 || num_classes < 1 || xyz_stride < 3 || batch_stride < 1 ||
      (batch_idx_bytes != 4 && batch_idx_bytes != 8) || (code_size != 8 && code_size != 10))
    return FSF_ERR_INVALID_ARG;
  if (!stats || !box_ptr || (n > 0 && (!cluster_xyz || !batch_idx || !labels || !bbox_targets || !bbox_weights || !assigned)))
    return FSF_ERR_INVALID_ARG;
  if (num_boxes > 0) {
    if (!boxes || !box_labels || (box_cols != 7 && box_cols != 9 && box_cols != 10) || box_stride < box_cols) return FSF_ERR_INVALID_ARG;
    if ((box_cols == 7) != (code_size == 8)) return FSF_ERR_INVALID_ARG;  // the coder appends box columns 7, 8 exactly when they exist
  }
  if (n >= ((int64_t)1 << 24) || num_boxes >= ((int64_t)1 << 24)) return FSF_ERR_UNSUPPORTED;  // (the f32 log scalars stay exact)
  FSF_CARVE(ClTargetsLayout, l, workspace, workspace_bytes, num_boxes, n);
  if (num_boxes > 0) {
    hipLaunchKernelGGL(cluster_box_prep_kernel, dim3((unsigned)fsf_cdiv(num_boxes, CL_BLOCK)), dim3(CL_BLOCK), 0, stream, boxes, num_boxes,
                       box_stride, enlarge_width, l.table, l.enc, l.box_hit);
    FSF_LAUNCH_CHECK();
  }
  if (l.nblk > 0) {
    if (batch_idx_bytes == 8)
      hipLaunchKernelGGL(cluster_targets_kernel<int64_t>, dim3((unsigned)l.nblk), dim3(CL_BLOCK), 0, stream, cluster_xyz, n, xyz_stride,
                         (const int64_t*)batch_idx, batch_stride, box_ptr, num_samples, boxes, box_stride, box_cols, l.table, l.enc, box_labels,
                         num_classes, code_size, labels, bbox_targets, bbox_weights, assigned, l.box_hit, l.partial);
    else
      hipLaunchKernelGGL(cluster_targets_kernel<int32_t>, dim3((unsigned)l.nblk), dim3(CL_BLOCK), 0, stream, cluster_xyz, n, xyz_stride,
                         (const int32_t*)batch_idx, batch_stride, box_ptr, num_samples, boxes, box_stride, box_cols, l.table, l.enc, box_labels,
                         num_classes, code_size, labels, bbox_targets, bbox_weights, assigned, l.box_hit, l.partial);
    FSF_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(cluster_targets_final_kernel, dim3(1), dim3(CL_BLOCK), 0, stream, l.partial, (int64_t)l.nblk, box_labels, l.box_hit, num_boxes,
                     n, l.nblk > 0, stats);
  FSF_LAUNCH_CHECK();
  return FSF_OK;
}

extern "C" int64_t fsf_cluster_loss_workspace_bytes(int64_t n) {
  if (n < 0) return -1;
  FsfArena arena = FsfArena::measure();
  cluster_loss_layout(arena, n);
  return arena.used;
}

extern "C" int fsf_cluster_loss_forward(const float* cls_logits, int64_t ld_cls, const float* reg_preds, int64_t ld_reg, int64_t n,
                                        int32_t num_classes, int32_t code_size, const int64_t* labels, const float* label_weights,
                                        const float* bbox_targets, const float* bbox_weights, const float* avg_factors, float gamma,
                                        float alpha, float w_cls, float w_center, float w_size, float w_rot, float w_vel, int32_t with_vel,
                                        void* workspace, int64_t workspace_bytes, float* losses, int64_t* counts, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const int st = cluster_loss_check(cls_logits, ld_cls, reg_preds, ld_reg, n, num_classes, code_size, labels, bbox_targets, bbox_weights,
                                    avg_factors);
  if (st != FSF_OK) return st;
  if (!losses || !counts || (with_vel && code_size != 10)) return FSF_ERR_INVALID_ARG;
  FsfArena arena(workspace, workspace_bytes);
  const int nblk = fsf_cdiv(n, CL_BLOCK);
  double* partials = cluster_loss_layout(arena, n);
  if (!arena.ok()) return FSF_ERR_WORKSPACE;
  if (nblk > 0) {
    hipLaunchKernelGGL(cluster_loss_partials_kernel, dim3((unsigned)nblk), dim3(CL_BLOCK), 0, stream, cls_logits, ld_cls, reg_preds, ld_reg,
                       n, num_classes, code_size, labels, label_weights, bbox_targets, bbox_weights, gamma, alpha, partials);
    FSF_LAUNCH_CHECK();
  }
  const ClusterLossWeights lw{gamma, alpha, w_cls, w_center, w_size, w_rot, w_vel};
  hipLaunchKernelGGL(cluster_loss_final_kernel, dim3(1), dim3(CL_BLOCK), 0, stream, partials, (int64_t)nblk, avg_factors, lw, with_vel != 0,
                     losses, counts);
  FSF_LAUNCH_CHECK();
  return FSF_OK;
}

extern "C" int fsf_cluster_loss_backward(const float* cls_logits, int64_t ld_cls, const float* reg_preds, int64_t ld_reg, int64_t n,
                                         int32_t num_classes, int32_t code_size, const int64_t* labels, const float* label_weights,
                                         const float* bbox_targets, const float* bbox_weights, const float* avg_factors, float gamma,
                                         float alpha, float w_cls, float w_center, float w_size, float w_rot, float w_vel,
                                         int32_t with_vel, const int64_t* counts, const float* grad_cls_loss, const float* grad_center_loss,
                                         const float* grad_size_loss, const float* grad_rot_loss, const float* grad_vel_loss,
                                         float* grad_cls_logits, float* grad_reg_preds, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const int st = cluster_loss_check(cls_logits, ld_cls, reg_preds, ld_reg, n, num_classes, code_size, labels, bbox_targets, bbox_weights,
                                    avg_factors);
  if (st != FSF_OK) return st;
  if (with_vel && code_size != 10) return FSF_ERR_INVALID_ARG;
  if (n == 0) return FSF_OK;
  if (!counts || !grad_cls_logits || !grad_reg_preds) return FSF_ERR_INVALID_ARG;
  const ClusterLossWeights lw{gamma, alpha, w_cls, w_center, w_size, w_rot, w_vel};
  const int grid = fsf_stream_grid(n * ((int64_t)num_classes + code_size), CL_BLOCK);
  hipLaunchKernelGGL(cluster_loss_backward_kernel, dim3((unsigned)grid), dim3(CL_BLOCK), 0, stream, cls_logits, ld_cls, reg_preds, ld_reg, n,
                     num_classes, code_size, labels, label_weights, bbox_targets, bbox_weights, avg_factors, lw, with_vel != 0, counts,
                     grad_cls_loss, grad_center_loss, grad_size_loss, grad_rot_loss, grad_vel_loss, grad_cls_logits, grad_reg_preds);
  FSF_LAUNCH_CHECK();
  return FSF_OK;
}
