// K35: the segmentation head's training targets and losses — see include/fsf_hip.h and docs/kernels/K35_seg_losses.md.
//   fsf_seg_targets        (K35a): points + per-sample GT boxes -> int64 labels, encoded vote targets, vote mask, masked count.
//                                  Three launches: per-box constants (one lane per box), one lane per point looping over its
//                                  sample's boxes (first hit wins), then one workgroup summing the per-workgroup counts.
//   fsf_seg_loss_forward   (K35b): weighted CE (mean over N) + L1 on the point's own class's vote columns (mean over 3 * n_valid).
//                                  One lane per row, fp64 per-workgroup partials, one final workgroup in fixed order.
//   fsf_seg_loss_backward  (K35c): dense grad_logits / grad_votes; the softmax is recomputed.  Per-row stats go to LDS, then the
//                                  workgroup writes its block of rows as one contiguous range.
// No float atomics and no host synchronisation: the same inputs give bit-identical outputs from run to run.
#include "box_contain.h"
#include "common.h"

namespace fsf {

constexpr int SL_BLOCK = 256;
constexpr int SL_BOX_WORDS = BOX_WORDS;  // (cx, cy, cz, half_w, half_l, half_h, cosa, sina): box_contain.h
constexpr int SL_FINAL_BLOCK = 256;

// ------------------------------------------------------------------------------------------------ K35a
// mmdet3d 0.x check_pt_in_box3d with the arithmetic pinned: cos / sin in float64 rounded once, cz = f32(z + h / 2).
__global__ void __launch_bounds__(SL_BLOCK) seg_box_prep_kernel(const float* __restrict__ boxes, int64_t num_boxes, int64_t box_stride,
                                                                float* __restrict__ table) {
  const int64_t k = (int64_t)blockIdx.x * SL_BLOCK + threadIdx.x;
  if (k >= num_boxes) return;
  const float* b = boxes + k * box_stride;
  box_constants(b[0], b[1], b[2], b[3], b[4], b[5], b[6], table + k * SL_BOX_WORDS);
}

template <typename BT>
__global__ void __launch_bounds__(SL_BLOCK) seg_targets_kernel(const float* __restrict__ points, int64_t n, int64_t pt_stride,
                                                               const BT* __restrict__ batch_idx, const int32_t* __restrict__ box_ptr,
                                                               int32_t num_samples, const float* __restrict__ table,
                                                               const int32_t* __restrict__ box_labels, int32_t num_classes,
                                                               int64_t* __restrict__ labels, float* __restrict__ targets,
                                                               uint8_t* __restrict__ mask, int32_t* __restrict__ partial_count) {
  __shared__ int32_t wave_count[SL_BLOCK / FSF_WAVE];
  const int64_t i = (int64_t)blockIdx.x * SL_BLOCK + threadIdx.x;
  int hit_count = 0;
  if (i < n) {
    const float* p = points + i * pt_stride;
    const float px = p[0], py = p[1], pz = p[2];
    const int64_t b = (int64_t)batch_idx[i];
    const int hit = (b >= 0 && b < num_samples) ? first_box_containing(px, py, pz, table, box_labels, box_ptr[b], box_ptr[b + 1]) : -1;
    float d[3] = {0.f, 0.f, 0.f};
    int64_t lab = num_classes;
    if (hit >= 0) {
      const float* t = table + (int64_t)hit * SL_BOX_WORDS;
      lab = box_labels[hit];
      const float g[3] = {t[0], t[1], t[2]};  // gravity centre: (x, y, f32(z_bottom + h / 2))
      const float q[3] = {px, py, pz};
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float dc = __fsub_rn(g[c], q[c]);
        const float s = (float)sqrt((double)fabsf(dc));  // correctly rounded: the f64 root of an f32 value, rounded once
        d[c] = dc > 0.f ? s : (dc < 0.f ? -s : 0.f);
      }
      hit_count = 1;
    }
    labels[i] = lab;
    targets[i * 3 + 0] = d[0];
    targets[i * 3 + 1] = d[1];
    targets[i * 3 + 2] = d[2];
    mask[i] = (uint8_t)hit_count;
  }
  const int wsum = fsf_wave_sum(hit_count);
  if (fsf_lane() == 0) wave_count[threadIdx.x / FSF_WAVE] = wsum;
  __syncthreads();
  if (threadIdx.x == 0) {
    int s = 0;
#pragma unroll
    for (int w = 0; w < SL_BLOCK / FSF_WAVE; ++w) s += wave_count[w];
    partial_count[blockIdx.x] = s;
  }
}

__global__ void __launch_bounds__(SL_FINAL_BLOCK) seg_count_final_kernel(const int32_t* __restrict__ partial, int64_t num_partials,
                                                                         int32_t* __restrict__ count) {
  __shared__ int32_t wave_count[SL_FINAL_BLOCK / FSF_WAVE];
  int s = 0;
  for (int64_t j = threadIdx.x; j < num_partials; j += SL_FINAL_BLOCK) s += partial[j];
  s = fsf_wave_sum(s);
  if (fsf_lane() == 0) wave_count[threadIdx.x / FSF_WAVE] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    int t = 0;
#pragma unroll
    for (int w = 0; w < SL_FINAL_BLOCK / FSF_WAVE; ++w) t += wave_count[w];
    *count = t;
  }
}

// ------------------------------------------------------------------------------------------------ K35b / K35c shared
// One row's logits: max and sum of exp(z - max) in fp32, in column order.  Rows whose stride and base allow it are read with
// 16-byte loads.
struct RowLse {
  float m, s;
};

__device__ __forceinline__ RowLse row_lse(const float* __restrict__ z, int c, bool vec4) {
  float m = -INFINITY;
  int j = 0;
  if (vec4) {
    for (; j + 4 <= c; j += 4) {
      const float4 q = *reinterpret_cast<const float4*>(z + j);
      m = fmaxf(m, fmaxf(fmaxf(q.x, q.y), fmaxf(q.z, q.w)));
    }
  }
  for (; j < c; ++j) m = fmaxf(m, z[j]);
  float s = 0.f;
  j = 0;
  if (vec4) {
    for (; j + 4 <= c; j += 4) {
      const float4 q = *reinterpret_cast<const float4*>(z + j);
      s += expf(q.x - m);
      s += expf(q.y - m);
      s += expf(q.z - m);
      s += expf(q.w - m);
    }
  }
  for (; j < c; ++j) s += expf(z[j] - m);
  return RowLse{m, s};
}

// ------------------------------------------------------------------------------------------------ K35b
// partials[block] = (sum of w[y] * (lse - z_y), sum of |v_y - t|) in fp64 and the block's masked-row count (as a double: exact).
__global__ void __launch_bounds__(SL_BLOCK) seg_loss_partials_kernel(const float* __restrict__ logits, int64_t ld_logits,
                                                                     const float* __restrict__ votes, int64_t ld_votes, int64_t n,
                                                                     int32_t num_classes, const int64_t* __restrict__ labels,
                                                                     const float* __restrict__ targets, const uint8_t* __restrict__ mask,
                                                                     const float* __restrict__ class_weight, bool vec4,
                                                                     double* __restrict__ partials) {
  __shared__ double wave_part[3][SL_BLOCK / FSF_WAVE];
  const int64_t i = (int64_t)blockIdx.x * SL_BLOCK + threadIdx.x;
  double ce = 0.0, l1 = 0.0, nv = 0.0;
  if (i < n) {
    const int64_t y = labels[i];
    if (y < 0 || y >= num_classes) {
      ce = NAN;  // a label outside [0, C) makes the loss NaN instead of reading past the row
    } else {
      const float* z = logits + i * ld_logits;
      const RowLse r = row_lse(z, num_classes, vec4);
      const float term = __fadd_rn(__fsub_rn(r.m, z[y]), logf(r.s));
      ce = (double)class_weight[y] * (double)term;
      if (mask[i]) {
        const float* v = votes + i * ld_votes + 3 * y;
        const float* t = targets + i * 3;
        l1 = (double)fabsf(__fsub_rn(v[0], t[0])) + (double)fabsf(__fsub_rn(v[1], t[1])) + (double)fabsf(__fsub_rn(v[2], t[2]));
        nv = 1.0;
      }
    }
  }
  ce = fsf_wave_sum(ce);
  l1 = fsf_wave_sum(l1);
  nv = fsf_wave_sum(nv);
  if (fsf_lane() == 0) {
    const int w = threadIdx.x / FSF_WAVE;
    wave_part[0][w] = ce;
    wave_part[1][w] = l1;
    wave_part[2][w] = nv;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < SL_BLOCK / FSF_WAVE; ++w) s += wave_part[threadIdx.x][w];
    partials[(int64_t)blockIdx.x * 3 + threadIdx.x] = s;
  }
}

__global__ void __launch_bounds__(SL_FINAL_BLOCK) seg_loss_final_kernel(const double* __restrict__ partials, int64_t num_partials,
                                                                        int64_t n, float ce_weight, float vote_weight,
                                                                        float* __restrict__ loss_ce, float* __restrict__ loss_vote,
                                                                        int64_t* __restrict__ counts) {
  __shared__ double wave_part[3][SL_FINAL_BLOCK / FSF_WAVE];
  double acc[3] = {0.0, 0.0, 0.0};
  for (int64_t j = threadIdx.x; j < num_partials; j += SL_FINAL_BLOCK) {
#pragma unroll
    for (int q = 0; q < 3; ++q) acc[q] += partials[j * 3 + q];
  }
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    const double s = fsf_wave_sum(acc[q]);
    if (fsf_lane() == 0) wave_part[q][threadIdx.x / FSF_WAVE] = s;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double t[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int q = 0; q < 3; ++q)
#pragma unroll
      for (int w = 0; w < SL_FINAL_BLOCK / FSF_WAVE; ++w) t[q] += wave_part[q][w];
    const int64_t n_valid = (int64_t)t[2];
    *loss_ce = (float)((double)ce_weight * (t[0] / (double)n));
    *loss_vote = n_valid > 0 ? (float)((double)vote_weight * (t[1] / (3.0 * (double)n_valid))) : 0.f;
    counts[0] = n;
    counts[1] = n_valid;
  }
}

// ------------------------------------------------------------------------------------------------ K35c
// grad_logits[i, c] = (softmax_c - [c == y]) * w[y] * ce_weight * g_ce / N
// grad_votes[i, j]  = sign(v_j - t_{j - 3y}) * vote_weight * g_vote / (3 * n_valid) for masked rows and 3y <= j < 3y + 3, else 0
__global__ void __launch_bounds__(SL_BLOCK) seg_loss_backward_kernel(const float* __restrict__ logits, int64_t ld_logits,
                                                                     const float* __restrict__ votes, int64_t ld_votes, int64_t n,
                                                                     int32_t num_classes, const int64_t* __restrict__ labels,
                                                                     const float* __restrict__ targets, const uint8_t* __restrict__ mask,
                                                                     const float* __restrict__ class_weight, float ce_weight,
                                                                     float vote_weight, const int64_t* __restrict__ counts,
                                                                     const float* __restrict__ grad_ce, const float* __restrict__ grad_vote,
                                                                     bool vec4, float* __restrict__ grad_logits,
                                                                     float* __restrict__ grad_votes) {
  __shared__ float row_m[SL_BLOCK], row_inv_s[SL_BLOCK], row_scale[SL_BLOCK];
  __shared__ int32_t row_y[SL_BLOCK];
  __shared__ float row_sign[SL_BLOCK][3];
  const int64_t row0 = (int64_t)blockIdx.x * SL_BLOCK;
  const int rows = (int)min((int64_t)SL_BLOCK, n - row0);
  const double n_all = (double)counts[0];
  const int64_t n_valid = counts[1];
  const float vote_scale = n_valid > 0 ? (float)((double)vote_weight * (double)grad_vote[0] / (3.0 * (double)n_valid)) : 0.f;
  const double ce_scale = (double)ce_weight * (double)grad_ce[0] / n_all;
  {
    const int r = threadIdx.x;
    if (r < rows) {
      const int64_t i = row0 + r;
      const int64_t y = labels[i];
      const bool ok = y >= 0 && y < num_classes;
      const RowLse s = row_lse(logits + i * ld_logits, num_classes, vec4);
      row_m[r] = s.m;
      row_inv_s[r] = 1.0f / s.s;
      row_y[r] = ok ? (int32_t)y : -1;
      row_scale[r] = ok ? (float)(ce_scale * (double)class_weight[y]) : NAN;
      float sg[3] = {0.f, 0.f, 0.f};
      if (ok && mask[i]) {
        const float* v = votes + i * ld_votes + 3 * y;
        const float* t = targets + i * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float d = __fsub_rn(v[c], t[c]);
          sg[c] = d > 0.f ? vote_scale : (d < 0.f ? -vote_scale : 0.f);
        }
      }
      row_sign[r][0] = sg[0];
      row_sign[r][1] = sg[1];
      row_sign[r][2] = sg[2];
    }
  }
  __syncthreads();
  // the block's rows are one contiguous range of each dense output: consecutive lanes write consecutive floats
  const int c = num_classes;
  const int nl = rows * c;  // <= 256 * 256: the checks cap num_classes at SL_BLOCK
  float* gl = grad_logits + row0 * c;
  for (int e = threadIdx.x; e < nl; e += SL_BLOCK) {
    const int r = e / c, j = e - r * c;
    const float p = expf(logits[(row0 + r) * ld_logits + j] - row_m[r]) * row_inv_s[r];
    gl[e] = __fmul_rn(p - (j == row_y[r] ? 1.f : 0.f), row_scale[r]);
  }
  const int c3 = 3 * c;
  const int nv = rows * c3;
  float* gv = grad_votes + row0 * c3;
  for (int e = threadIdx.x; e < nv; e += SL_BLOCK) {
    const int r = e / c3, j = e - r * c3;
    const int k = j - 3 * row_y[r];
    gv[e] = (row_y[r] >= 0 && k >= 0 && k < 3) ? row_sign[r][k] : 0.f;
  }
}

static inline bool rows_vec4(const float* p, int64_t ld) { return ((uintptr_t)p & 15u) == 0 && ld % 4 == 0; }

}  // namespace fsf

using namespace fsf;

struct SegTargetsLayout {
  int nblk;
  float* table;
  int32_t* partial;
  SegTargetsLayout(FsfArena& arena, int64_t num_boxes, int64_t n)
      : nblk(fsf_cdiv(n, SL_BLOCK)), table(arena.take<float>(SL_BOX_WORDS * num_boxes)), partial(arena.take<int32_t>(nblk)) {}
};
// (one slice: a function in place of a layout struct, taken from a hand-made arena in the entry)
static double* seg_loss_layout(FsfArena& arena, int64_t n) { return arena.take<double>(3 * (int64_t)fsf_cdiv(n, SL_BLOCK)); }

extern "C" int64_t fsf_seg_targets_workspace_bytes(int64_t num_boxes, int64_t n) {
  if (num_boxes < 0 || n < 0) return -1;
  return fsf_layout_bytes<SegTargetsLayout>(num_boxes, n);
}

extern "C" int fsf_seg_targets(const float* points, int64_t n, int64_t pt_stride, const void* batch_idx, int32_t batch_idx_bytes,
                               const int32_t* box_ptr, int32_t num_samples, const float* boxes, int64_t num_boxes, int64_t box_stride,
                               const int32_t* box_labels, int32_t num_classes, void* workspace, int64_t workspace_bytes,
                               int64_t* labels, float* targets, uint8_t* mask, int32_t* count, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (n < 0 || num_samples < 0 || num_boxes < 0 || num_classes < 1 || pt_stride < 3 || (batch_idx_bytes != 4 && batch_idx_bytes != 8))
    return FSF_ERR_INVALID_ARG;
  if (!count || !box_ptr || (n > 0 && (!points || !batch_idx || !labels || !targets || !mask))) return FSF_ERR_INVALID_ARG;
  if (num_boxes > 0 && (!boxes || !box_labels || box_stride < 7)) return FSF_ERR_INVALID_ARG;
  if (n >= ((int64_t)1 << 40) || num_boxes >= ((int64_t)1 << 31)) return FSF_ERR_UNSUPPORTED;
  FSF_CARVE(SegTargetsLayout, l, workspace, workspace_bytes, num_boxes, n);
  if (num_boxes > 0) {
    hipLaunchKernelGGL(seg_box_prep_kernel, dim3((unsigned)fsf_cdiv(num_boxes, SL_BLOCK)), dim3(SL_BLOCK), 0, stream, boxes, num_boxes,
                       box_stride, l.table);
    FSF_LAUNCH_CHECK();
  }
  if (l.nblk > 0) {
    if (batch_idx_bytes == 8)
      hipLaunchKernelGGL(seg_targets_kernel<int64_t>, dim3((unsigned)l.nblk), dim3(SL_BLOCK), 0, stream, points, n, pt_stride,
                         (const int64_t*)batch_idx, box_ptr, num_samples, l.table, box_labels, num_classes, labels, targets, mask, l.partial);
    else
      hipLaunchKernelGGL(seg_targets_kernel<int32_t>, dim3((unsigned)l.nblk), dim3(SL_BLOCK), 0, stream, points, n, pt_stride,
                         (const int32_t*)batch_idx, box_ptr, num_samples, l.table, box_labels, num_classes, labels, targets, mask, l.partial);
    FSF_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(seg_count_final_kernel, dim3(1), dim3(SL_FINAL_BLOCK), 0, stream, l.partial, (int64_t)l.nblk, count);
  FSF_LAUNCH_CHECK();
  return FSF_OK;
}

extern "C" int64_t fsf_seg_loss_workspace_bytes(int64_t n) {
  if (n < 0) return -1;
  FsfArena arena = FsfArena::measure();
  seg_loss_layout(arena, n);
  return arena.used;
}

static int seg_loss_check(const float* logits, int64_t ld_logits, const float* votes, int64_t ld_votes, int64_t n, int32_t num_classes,
                          const int64_t* labels, const float* targets, const uint8_t* mask, const float* class_weight) {
  if (n < 0 || num_classes < 1 || ld_logits < num_classes || ld_votes < 3 * (int64_t)num_classes) return FSF_ERR_INVALID_ARG;
  if (n > 0 && (!logits || !votes || !labels || !targets || !mask || !class_weight)) return FSF_ERR_INVALID_ARG;
  if (num_classes > SL_BLOCK || n >= ((int64_t)1 << 40)) return FSF_ERR_UNSUPPORTED;
  return FSF_OK;
}

extern "C" int fsf_seg_loss_forward(const float* logits, int64_t ld_logits, const float* votes, int64_t ld_votes, int64_t n,
                                    int32_t num_classes, const int64_t* labels, const float* targets, const uint8_t* mask,
                                    const float* class_weight, float ce_weight, float vote_weight, void* workspace,
                                    int64_t workspace_bytes, float* loss_ce, float* loss_vote, int64_t* counts, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const int st = seg_loss_check(logits, ld_logits, votes, ld_votes, n, num_classes, labels, targets, mask, class_weight);
  if (st != FSF_OK) return st;
  if (!loss_ce || !loss_vote || !counts) return FSF_ERR_INVALID_ARG;
  FsfArena arena(workspace, workspace_bytes);
  const int nblk = fsf_cdiv(n, SL_BLOCK);
  double* partials = seg_loss_layout(arena, n);
  if (!arena.ok()) return FSF_ERR_WORKSPACE;
  if (nblk > 0) {
    hipLaunchKernelGGL(seg_loss_partials_kernel, dim3((unsigned)nblk), dim3(SL_BLOCK), 0, stream, logits, ld_logits, votes, ld_votes, n,
                       num_classes, labels, targets, mask, class_weight, rows_vec4(logits, ld_logits), partials);
    FSF_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(seg_loss_final_kernel, dim3(1), dim3(SL_FINAL_BLOCK), 0, stream, partials, (int64_t)nblk, n, ce_weight, vote_weight,
                     loss_ce, loss_vote, counts);
  FSF_LAUNCH_CHECK();
  return FSF_OK;
}

extern "C" int fsf_seg_loss_backward(const float* logits, int64_t ld_logits, const float* votes, int64_t ld_votes, int64_t n,
                                     int32_t num_classes, const int64_t* labels, const float* targets, const uint8_t* mask,
                                     const float* class_weight, float ce_weight, float vote_weight, const int64_t* counts,
                                     const float* grad_ce, const float* grad_vote, float* grad_logits, float* grad_votes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const int st = seg_loss_check(logits, ld_logits, votes, ld_votes, n, num_classes, labels, targets, mask, class_weight);
  if (st != FSF_OK) return st;
  if (n == 0) return FSF_OK;
  if (!counts || !grad_ce || !grad_vote || !grad_logits || !grad_votes) return FSF_ERR_INVALID_ARG;
  hipLaunchKernelGGL(seg_loss_backward_kernel, dim3((unsigned)fsf_cdiv(n, SL_BLOCK)), dim3(SL_BLOCK), 0, stream, logits, ld_logits, votes,
                     ld_votes, n, num_classes, labels, targets, mask, class_weight, ce_weight, vote_weight, counts, grad_ce, grad_vote,
                     rows_vec4(logits, ld_logits), grad_logits, grad_votes);
  FSF_LAUNCH_CHECK();
  return FSF_OK;
}
