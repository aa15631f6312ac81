// The query heads' box encoding (BasePointBBoxCoder.encode with the arithmetic pinned, docs/kernels/K36_cluster_losses.md), shared by
// K36a (cluster_loss.hip: point-in-box assignment), K37b and K38 (hybrid_assign.hip: 3-D / 2-D hybrid assignment, and the refine heads'
// with the distance step): one definition of the per-box encoded values and of the label / target / weight rows a query gets from the
// box it was assigned.
#pragma once
#include "common.h"

namespace fsf {

constexpr int CL_ENC_WORDS = 8;  // (log w, log l, log h, sin yaw, cos yaw, -, -, -)

// Per box: the coder's log(dim + 1e-6) / sin / cos (float64 functions of f32 values, rounded once).
__device__ __forceinline__ void cluster_encode_box(const float* __restrict__ b, float* __restrict__ t) {
#pragma unroll
  for (int c = 0; c < 3; ++c) t[c] = (float)log((double)__fadd_rn(b[3 + c], 1e-6f));
  t[3] = (float)sin((double)b[6]);
  t[4] = (float)cos((double)b[6]);
}

// Row i of labels / bbox_targets / bbox_weights for the query at q assigned box `hit` (an index into boxes / enc / box_labels, -1:
// background).  Sets the box's hit flag (every writer stores the same word).  Returns 1 for a positive row.
__device__ __forceinline__ int cluster_write_target_rows(int64_t i, const float* q, int hit, const float* __restrict__ boxes,
                                                         int64_t box_stride, int32_t box_cols, const float* __restrict__ enc,
                                                         const int32_t* __restrict__ box_labels, int32_t num_classes, int32_t code_size,
                                                         int64_t* __restrict__ labels, float* __restrict__ bbox_targets,
                                                         float* __restrict__ bbox_weights, int32_t* __restrict__ box_hit) {
  float tgt[10], wgt[10];
#pragma unroll
  for (int c = 0; c < 10; ++c) tgt[c] = wgt[c] = 0.f;
  int64_t lab = num_classes;
  if (hit >= 0) {
    const float* g = boxes + (int64_t)hit * box_stride;
    const float* t = enc + (int64_t)hit * CL_ENC_WORDS;
    lab = box_labels[hit];
#pragma unroll
    for (int c = 0; c < 3; ++c) tgt[c] = __fsub_rn(g[c], q[c]);  // the coder's centre delta: box columns 0..2 as stored
#pragma unroll
    for (int c = 0; c < 5; ++c) tgt[3 + c] = t[c];
#pragma unroll
    for (int c = 0; c < 10; ++c) wgt[c] = 1.f;
    if (code_size == 10) {
      tgt[8] = g[7];
      tgt[9] = g[8];
      if (box_cols == 10) wgt[8] = wgt[9] = g[9];  // the copy-paste flag switches the velocity columns off
    }
    box_hit[hit] = 1;
  }
  labels[i] = lab;
  float* to = bbox_targets + i * code_size;
  float* wo = bbox_weights + i * code_size;
  if (code_size == 10) {
#pragma unroll
    for (int c = 0; c < 10; ++c) {
      to[c] = tgt[c];
      wo[c] = wgt[c];
    }
  } else {
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      to[c] = tgt[c];
      wo[c] = wgt[c];
    }
  }
  return hit >= 0 ? 1 : 0;
}

// Sum of one int per lane over a workgroup of `BLOCK` lanes -> partial[blockIdx.x] (lane 0 writes).
template <int BLOCK>
__device__ __forceinline__ void cluster_block_count(int v, int32_t* __restrict__ partial) {
  __shared__ int32_t wave_count[BLOCK / FSF_WAVE];
  const int wsum = fsf_wave_sum(v);
  if (fsf_lane() == 0) wave_count[threadIdx.x / FSF_WAVE] = wsum;
  __syncthreads();
  if (threadIdx.x == 0) {
    int s = 0;
#pragma unroll
    for (int w = 0; w < BLOCK / FSF_WAVE; ++w) s += wave_count[w];
    partial[blockIdx.x] = s;
  }
}

// stats = (num_preds, num_pos_preds, num_gts, assigned_gts, cls_avg_factor, reg_avg_factor), all f32 (integers below 2^24 are exact),
// by one workgroup of `BLOCK` lanes: the per-workgroup positive counts, the boxes with a label >= 0 and the boxes that were hit.
template <int BLOCK>
__device__ __forceinline__ void cluster_stats_final(const int32_t* __restrict__ partial, int64_t num_partials,
                                                    const int32_t* __restrict__ box_labels, const int32_t* __restrict__ box_hit,
                                                    int64_t num_boxes, int64_t n, bool hits_valid, float* __restrict__ stats) {
  __shared__ int32_t wave_count[3][BLOCK / FSF_WAVE];
  int acc[3] = {0, 0, 0};
  for (int64_t j = threadIdx.x; j < num_partials; j += BLOCK) acc[0] += partial[j];
  for (int64_t k = threadIdx.x; k < num_boxes; k += BLOCK) {
    acc[1] += box_labels[k] >= 0 ? 1 : 0;
    acc[2] += (hits_valid && box_hit[k] != 0) ? 1 : 0;
  }
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    const int s = fsf_wave_sum(acc[q]);
    if (fsf_lane() == 0) wave_count[q][threadIdx.x / FSF_WAVE] = s;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int t[3] = {0, 0, 0};
#pragma unroll
    for (int q = 0; q < 3; ++q)
#pragma unroll
      for (int w = 0; w < BLOCK / FSF_WAVE; ++w) t[q] += wave_count[q][w];
    stats[0] = (float)n;
    stats[1] = (float)t[0];
    stats[2] = (float)t[1];
    stats[3] = (float)t[2];
    stats[4] = (float)n;
    stats[5] = (float)t[0];
  }
}

}  // namespace fsf
