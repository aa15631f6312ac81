// K37: the camera-query head's hybrid 3-D / 2-D target assignment — see include/fsf_hip.h and docs/kernels/K37_hybrid_assign.md.
//   fsf_gt_boxes_2d   (K37a): per (un-augmented GT box, camera) the eight corners of the solid box_contain.h tests, projected with the
//                             sample's lidar2img (project.hip's row product), clipped against the image canvas in fp64 -> the f32 2-D box
//                             and a keep flag.  One lane per (box, camera), one launch.
//   fsf_hybrid_assign (K37b): per query: the first augmented GT box containing its centre (K36a's rule), else MaxIoUAssigner on the 2-D
//                             boxes of its camera (maximum IoU >= pos_iou_thr, overridden by the low-quality pass), then K36a's label /
//                             target / weight rows, hit flags and stats.  Four launches: per-box constants, one wave per (box, camera)
//                             for the box's maximum IoU over its camera's queries, one lane per query, one final workgroup.
//   fsf_frustum_assign (K38): K37b with the refine heads' third step folded into the per-query kernel (a template flag): a query that
//                             neither step assigned takes the nearest GT, in BEV, of the class the previous stage predicted for it,
//                             when that GT is closer than the class's radius.  Same four launches; docs/kernels/K38_frustum_assign.md.
// No float atomics, no memset, no host synchronisation: the same inputs give bit-identical outputs from run to run.
#include "box_contain.h"
#include "cluster_encode.h"
#include "common.h"

namespace fsf {

constexpr int HY_BLOCK = 256;
constexpr int HY_MAX_CAMS = 64;

// Sample whose CSR range [box_ptr[b], box_ptr[b + 1]) holds row k, -1 when none does.
__device__ __forceinline__ int hy_sample_of(const int32_t* __restrict__ box_ptr, int32_t num_samples, int64_t k) {
  for (int b = 0; b < num_samples; ++b)
    if (k >= box_ptr[b] && k < box_ptr[b + 1]) return b;
  return -1;
}

// pts_4d @ lidar2img^T for one output row, as project.hip evaluates it: an fma chain in k order.
__device__ __forceinline__ float hy_proj_row(const float* __restrict__ m, float x, float y, float z) {
  float acc = __fmul_rn(x, m[0]);
  acc = __fmaf_rn(y, m[1], acc);
  acc = __fmaf_rn(z, m[2], acc);
  acc = __fmaf_rn(1.0f, m[3], acc);
  return acc;
}

struct HyExtent {
  double x0, y0, x1, y1;
  bool any;
  __device__ __forceinline__ void add(double x, double y) {
    x0 = any ? fmin(x0, x) : x;
    y0 = any ? fmin(y0, y) : y;
    x1 = any ? fmax(x1, x) : x;
    y1 = any ? fmax(y1, y) : y;
    any = true;
  }
};

// Liang-Barsky clip of the segment a -> b against [0, W] x [0, H]; the clipped end points join the extent.  An end point that
// survives (t = 0 / t = 1) is taken as it is, any other as a + t * (b - a) clamped onto the canvas; every operation a separately
// rounded fp64 one.
__device__ __forceinline__ void hy_clip_segment(double ax, double ay, double bx, double by, double W, double H, HyExtent& e) {
  const double dx = __dsub_rn(bx, ax), dy = __dsub_rn(by, ay);
  const double p[4] = {-dx, dx, -dy, dy};
  const double q[4] = {ax, __dsub_rn(W, ax), ay, __dsub_rn(H, ay)};
  double t0 = 0.0, t1 = 1.0;
  bool ok = true;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    if (!ok) continue;
    if (p[s] == 0.0) {
      if (q[s] < 0.0) ok = false;
    } else {
      const double r = __ddiv_rn(q[s], p[s]);
      if (p[s] < 0.0) {
        if (r > t1) ok = false;
        else t0 = fmax(t0, r);
      } else {
        if (r < t0) ok = false;
        else t1 = fmin(t1, r);
      }
    }
  }
  if (!ok) return;
  // (an interpolated point lies inside the canvas up to its rounding: clamped onto it)
  if (t0 == 0.0) e.add(ax, ay);
  else e.add(fmin(fmax(__dadd_rn(ax, __dmul_rn(t0, dx)), 0.0), W), fmin(fmax(__dadd_rn(ay, __dmul_rn(t0, dy)), 0.0), H));
  if (t1 == 1.0) e.add(bx, by);
  else e.add(fmin(fmax(__dadd_rn(ax, __dmul_rn(t1, dx)), 0.0), W), fmin(fmax(__dadd_rn(ay, __dmul_rn(t1, dy)), 0.0), H));
}

__device__ __forceinline__ double hy_cross(double ax, double ay, double bx, double by, double px, double py) {
  return __dsub_rn(__dmul_rn(__dsub_rn(bx, ax), __dsub_rn(py, ay)), __dmul_rn(__dsub_rn(by, ay), __dsub_rn(px, ax)));
}

// ------------------------------------------------------------------------------------------------ K37a
__global__ void __launch_bounds__(HY_BLOCK) gt_boxes_2d_kernel(const float* __restrict__ boxes, int64_t num_boxes, int64_t box_stride,
                                                               const int32_t* __restrict__ box_labels, const int32_t* __restrict__ box_ptr,
                                                               int32_t num_samples, const float* __restrict__ lidar2img, int32_t ncam,
                                                               float canvas_w, float canvas_h, float* __restrict__ boxes_2d,
                                                               int32_t* __restrict__ keep) {
  const int64_t t = (int64_t)blockIdx.x * HY_BLOCK + threadIdx.x;
  if (t >= num_boxes * ncam) return;
  const int64_t k = t / ncam;
  const int cam = (int)(t - k * ncam);
  float out[4] = {0.f, 0.f, 0.f, 0.f};
  int kept = 0;
  const int b = box_labels[k] >= 0 ? hy_sample_of(box_ptr, num_samples, k) : -1;
  if (b >= 0) {
    const float* g = boxes + k * box_stride;
    const float x = g[0], y = g[1], z = g[2], hw = g[3] * 0.5f, hl = g[4] * 0.5f, zt = __fadd_rn(g[2], g[5]);
    const float c = (float)cos((double)g[6]), s = (float)sin((double)g[6]);
    const float* m = lidar2img + ((int64_t)b * ncam + cam) * 16;
    double px[8], py[8];
    bool valid = false;
#pragma unroll
    for (int v = 0; v < 8; ++v) {
      const float dx = (v & 4) ? hl : -hl, dy = (v & 2) ? hw : -hw;
      const float X = __fsub_rn(__fadd_rn(x, __fmul_rn(dx, c)), __fmul_rn(dy, s));
      const float Y = __fadd_rn(__fadd_rn(y, __fmul_rn(dx, s)), __fmul_rn(dy, c));
      const float Z = (v & 1) ? zt : z;
      const float u = hy_proj_row(m, X, Y, Z), w = hy_proj_row(m + 4, X, Y, Z);
      float d = hy_proj_row(m + 8, X, Y, Z);
      valid |= d > 1e-5f;
      d = fminf(fmaxf(d, 1e-5f), 1e5f);
      px[v] = (double)__fdiv_rn(u, d);
      py[v] = (double)__fdiv_rn(w, d);
    }
    if (valid) {
      const double W = (double)canvas_w, H = (double)canvas_h;
      HyExtent e{0.0, 0.0, 0.0, 0.0, false};
      for (int i = 0; i < 8; ++i)
        for (int j = i + 1; j < 8; ++j) hy_clip_segment(px[i], py[i], px[j], py[j], W, H, e);
      for (int q = 0; q < 4; ++q) {  // canvas corners inside a triangle of the eight points
        const double cx = (q == 1 || q == 2) ? W : 0.0, cy = (q >= 2) ? H : 0.0;
        bool inside = false;
        for (int i = 0; i < 8 && !inside; ++i)
          for (int j = i + 1; j < 8 && !inside; ++j)
            for (int l = j + 1; l < 8 && !inside; ++l) {
              const double d1 = hy_cross(px[i], py[i], px[j], py[j], cx, cy);
              const double d2 = hy_cross(px[j], py[j], px[l], py[l], cx, cy);
              const double d3 = hy_cross(px[l], py[l], px[i], py[i], cx, cy);
              const bool pos = d1 >= 0.0 && d2 >= 0.0 && d3 >= 0.0, neg = d1 <= 0.0 && d2 <= 0.0 && d3 <= 0.0;
              inside = (pos || neg) && !(d1 == 0.0 && d2 == 0.0 && d3 == 0.0);
            }
        if (inside) e.add(cx, cy);
      }
      if (e.any && e.x1 > e.x0 && e.y1 > e.y0) {
        kept = 1;
        out[0] = (float)e.x0;
        out[1] = (float)e.y0;
        out[2] = (float)e.x1;
        out[3] = (float)e.y1;
      }
    }
  }
  *reinterpret_cast<float4*>(boxes_2d + t * 4) = make_float4(out[0], out[1], out[2], out[3]);
  keep[t] = kept;
}

// ------------------------------------------------------------------------------------------------ K37b
// mmdet 2.14 bbox_overlaps(mode='iou'), f32, every operation rounded separately: no +1, sides clamped at 0, union floored at 1e-6.
__device__ __forceinline__ float hy_iou(const float4 g, const float4 d) {
  const float area_g = __fmul_rn(__fsub_rn(g.z, g.x), __fsub_rn(g.w, g.y));
  const float area_d = __fmul_rn(__fsub_rn(d.z, d.x), __fsub_rn(d.w, d.y));
  const float w = fmaxf(__fsub_rn(fminf(g.z, d.z), fmaxf(g.x, d.x)), 0.f);
  const float h = fmaxf(__fsub_rn(fminf(g.w, d.w), fmaxf(g.y, d.y)), 0.f);
  const float overlap = __fmul_rn(w, h);
  const float uni = fmaxf(__fsub_rn(__fadd_rn(area_g, area_d), overlap), 1e-6f);
  return __fdiv_rn(overlap, uni);
}

// The camera of a query: preds_2d column 6 when it is an integer in [0, ncam), else -1.
__device__ __forceinline__ int hy_query_cam(const float* __restrict__ p, int32_t ncam) {
  const float v = p[6];
  if (!(v >= 0.f && v < (float)ncam)) return -1;
  const int c = (int)v;
  return (float)c == v ? c : -1;
}

__global__ void __launch_bounds__(HY_BLOCK) hybrid_box_prep_kernel(const float* __restrict__ boxes, int64_t num_boxes, int64_t box_stride,
                                                                   float extra_height, float* __restrict__ table, float* __restrict__ enc,
                                                                   int32_t* __restrict__ box_hit) {
  const int64_t k = (int64_t)blockIdx.x * HY_BLOCK + threadIdx.x;
  if (k >= num_boxes) return;
  const float* b = boxes + k * box_stride;
  box_constants(b[0], b[1], __fsub_rn(b[2], extra_height), b[3], b[4], __fadd_rn(b[5], __fmul_rn(extra_height, 2.0f)), b[6],
                table + k * BOX_WORDS);
  cluster_encode_box(b, enc + k * CL_ENC_WORDS);
  box_hit[k] = 0;
}

// One wave per (2-D box, camera): the box's maximum IoU over the queries of its sample and camera, -1 when it was dropped or no query
// is there.  A maximum does not depend on the order of its operands.
template <typename BT>
__global__ void __launch_bounds__(HY_BLOCK) hybrid_gt_max_kernel(const float* __restrict__ preds_2d, int64_t n, int64_t preds_stride,
                                                                 const BT* __restrict__ batch_idx, int64_t batch_stride,
                                                                 const int32_t* __restrict__ box_ptr_2d, int32_t num_samples,
                                                                 const float* __restrict__ boxes_2d, const int32_t* __restrict__ keep_2d,
                                                                 int64_t num_pairs, int32_t ncam, float* __restrict__ gt_max) {
  const int64_t t = (int64_t)blockIdx.x * (HY_BLOCK / FSF_WAVE) + threadIdx.x / FSF_WAVE;
  if (t >= num_pairs) return;  // (whole waves leave together)
  const int64_t k = t / ncam;
  const int cam = (int)(t - k * ncam);
  float best = -1.f;
  const int b = keep_2d[t] != 0 ? hy_sample_of(box_ptr_2d, num_samples, k) : -1;
  if (b >= 0) {
    const float4 g = *reinterpret_cast<const float4*>(boxes_2d + t * 4);
    for (int64_t i = fsf_lane(); i < n; i += FSF_WAVE) {
      if ((int64_t)batch_idx[i * batch_stride] != b) continue;
      const float* p = preds_2d + i * preds_stride;
      if (hy_query_cam(p, ncam) != cam) continue;
      best = fmaxf(best, hy_iou(g, make_float4(p[0], p[1], p[2], p[3])));
    }
  }
  best = fsf_wave_max(best);
  if (fsf_lane() == 0) gt_max[t] = best;
}

// EXT (K38): the distance step for the queries both steps left unassigned (when class_max_dist is given) and the per-query source
// (when `source` is given).  Without EXT the branches are compiled out: K37b's results and register / scratch figures.
template <typename BT, bool EXT>
__global__ void __launch_bounds__(HY_BLOCK) hybrid_assign_kernel(
    const float* __restrict__ xyz, int64_t n, int64_t xyz_stride, const BT* __restrict__ batch_idx, int64_t batch_stride,
    const float* __restrict__ preds_2d, int64_t preds_stride, const int32_t* __restrict__ box_ptr_2d, const float* __restrict__ boxes_2d,
    const int32_t* __restrict__ keep_2d, const float* __restrict__ gt_max, int64_t num_boxes_2d, int32_t ncam,
    const int32_t* __restrict__ box_ptr, int32_t num_samples, const float* __restrict__ boxes, int64_t num_boxes, int64_t box_stride,
    int32_t box_cols, const float* __restrict__ table, const float* __restrict__ enc, const int32_t* __restrict__ box_labels,
    int32_t num_classes, int32_t code_size, float pos_iou_thr, float min_pos_iou, int64_t* __restrict__ labels,
    float* __restrict__ bbox_targets, float* __restrict__ bbox_weights, int32_t* __restrict__ assigned, int32_t* __restrict__ box_hit,
    int32_t* __restrict__ partial_count, const float* __restrict__ old_cls_logits, int64_t logits_stride,
    const float* __restrict__ class_max_dist, int32_t* __restrict__ source) {
  const int64_t i = (int64_t)blockIdx.x * HY_BLOCK + threadIdx.x;
  int hit_count = 0;
  if (i < n) {
    const float* p = xyz + i * xyz_stride;
    const float q[3] = {p[0], p[1], p[2]};
    const int64_t b = (int64_t)batch_idx[i * batch_stride];
    int k0 = 0;
    int hit = -1;
    int src = 0;  // 0 none, 1 3-D, 2 2-D, 3 distance
    if (b >= 0 && b < num_samples) {
      k0 = box_ptr[b];
      const int k1 = box_ptr[b + 1] < num_boxes ? box_ptr[b + 1] : (int)num_boxes;
      if (k0 >= 0) hit = first_box_containing(q[0], q[1], q[2], table, box_labels, k0, k1);  // 3-D wins
      if (EXT && hit >= 0) src = 1;
      const float* d = preds_2d + i * preds_stride;
      const int cam = hy_query_cam(d, ncam);
      if (hit < 0 && k0 >= 0 && cam >= 0) {
        const float4 dt = make_float4(d[0], d[1], d[2], d[3]);
        const int j0 = box_ptr_2d[b] > 0 ? box_ptr_2d[b] : 0;
        const int j1 = box_ptr_2d[b + 1] < num_boxes_2d ? box_ptr_2d[b + 1] : (int)num_boxes_2d;
        float best = -1.f;
        int arg = -1, low = -1;
        for (int j = j0; j < j1; ++j) {
          const int64_t t = (int64_t)j * ncam + cam;
          if (keep_2d[t] == 0) continue;
          const float v = hy_iou(*reinterpret_cast<const float4*>(boxes_2d + t * 4), dt);
          if (v > best) {  // strict: the first maximum wins
            best = v;
            arg = j;
          }
          const float gm = gt_max[t];
          if (gm >= min_pos_iou && v == gm) low = j;  // low-quality pass, ascending: the last claim stands
        }
        const int j = low >= 0 ? low : ((arg >= 0 && best >= pos_iou_thr) ? arg : -1);
        if (j >= 0) {  // index k inside the un-augmented list -> row k of the augmented one, background when that row does not exist
          const int k = k0 + (j - j0);
          if (k < k1 && box_labels[k] >= 0) {
            hit = k;
            if (EXT) src = 2;
          }
        }
      }
      if (EXT && class_max_dist != nullptr && hit < 0 && k0 >= 0) {
        // the class the previous stage predicted: strict > from column 0 (the lowest index wins a tie; a row of NaN gives class 0)
        const float* lg = old_cls_logits + i * logits_stride;
        int c = 0;
        float top = lg[0];
        for (int j = 1; j < num_classes; ++j) {
          const float v = lg[j];
          if (v > top) {
            top = v;
            c = j;
          }
        }
        const float radius = class_max_dist[c];
        float near = __builtin_inff();
        int arg = -1;
        for (int k = k0; k < k1; ++k) {  // the first row of minimum BEV distance among the sample's rows of that class
          if (box_labels[k] != c) continue;
          const float* g = boxes + (int64_t)k * box_stride;
          const float dx = __fsub_rn(q[0], g[0]), dy = __fsub_rn(q[1], g[1]);
          // sqrtf, not __fsqrt_rn: without OCML_BASIC_ROUNDED_OPERATIONS that intrinsic is the bare 1-ulp hardware root, while
          // sqrtf is compiled to the correctly rounded sequence (the host's root, bit for bit)
          const float d = sqrtf(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)));
          if (d < near) {  // (a NaN or infinite distance never wins)
            near = d;
            arg = k;
          }
        }
        if (arg >= 0 && near < radius) {
          hit = arg;
          src = 3;
        }
      }
    }
    hit_count = cluster_write_target_rows(i, q, hit, boxes, box_stride, box_cols, enc, box_labels, num_classes, code_size, labels,
                                          bbox_targets, bbox_weights, box_hit);
    assigned[i] = hit >= 0 ? hit - k0 : -1;
    if (EXT && source != nullptr) source[i] = src;
  }
  cluster_block_count<HY_BLOCK>(hit_count, partial_count);
}

__global__ void __launch_bounds__(HY_BLOCK) hybrid_assign_final_kernel(const int32_t* __restrict__ partial, int64_t num_partials,
                                                                       const int32_t* __restrict__ box_labels,
                                                                       const int32_t* __restrict__ box_hit, int64_t num_boxes, int64_t n,
                                                                       bool hits_valid, float* __restrict__ stats) {
  cluster_stats_final<HY_BLOCK>(partial, num_partials, box_labels, box_hit, num_boxes, n, hits_valid, stats);
}

}  // namespace fsf

using namespace fsf;

extern "C" int fsf_gt_boxes_2d(const float* boxes, int64_t num_boxes, int64_t box_stride, const int32_t* box_labels,
                               const int32_t* box_ptr, int32_t num_samples, const float* lidar2img, int32_t ncam, float canvas_w,
                               float canvas_h, float* boxes_2d, int32_t* keep, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (num_boxes < 0 || num_samples < 0 || ncam < 1 || ncam > HY_MAX_CAMS || !box_ptr || !(canvas_w > 0.f) || !(canvas_h > 0.f))
    return FSF_ERR_INVALID_ARG;
  if (num_boxes > 0 && (!boxes || !box_labels || !lidar2img || !boxes_2d || !keep || box_stride < 7 || num_samples < 1))
    return FSF_ERR_INVALID_ARG;
  if (num_boxes >= ((int64_t)1 << 24) || ((uintptr_t)boxes_2d % 16) != 0) return FSF_ERR_UNSUPPORTED;
  if (num_boxes == 0) return FSF_OK;
  hipLaunchKernelGGL(gt_boxes_2d_kernel, dim3((unsigned)fsf_cdiv(num_boxes * ncam, HY_BLOCK)), dim3(HY_BLOCK), 0, stream, boxes, num_boxes,
                     box_stride, box_labels, box_ptr, num_samples, lidar2img, ncam, canvas_w, canvas_h, boxes_2d, keep);
  FSF_LAUNCH_CHECK();
  return FSF_OK;
}

struct HyLayout {
  int nblk;
  float *table, *enc;
  int32_t *box_hit, *partial;
  float* gt_max;
  HyLayout(FsfArena& arena, int64_t num_boxes, int64_t pairs, int64_t n)
      : nblk(fsf_cdiv(n, HY_BLOCK)), table(arena.take<float>(BOX_WORDS * num_boxes)), enc(arena.take<float>(CL_ENC_WORDS * num_boxes)),
        box_hit(arena.take<int32_t>(num_boxes)), partial(arena.take<int32_t>(nblk)), gt_max(arena.take<float>(pairs)) {}
};

extern "C" int64_t fsf_hybrid_assign_workspace_bytes(int64_t num_boxes, int64_t num_boxes_2d, int32_t ncam, int64_t n) {
  if (num_boxes < 0 || num_boxes_2d < 0 || ncam < 1 || n < 0) return -1;
  return fsf_layout_bytes<HyLayout>(num_boxes, num_boxes_2d * ncam, n);
}

// K37b and K38 share everything: `ext` selects the per-query kernel with the distance step and the source output.
static int hybrid_assign_run(const float* cluster_xyz, int64_t n, int64_t xyz_stride, const void* batch_idx, int32_t batch_idx_bytes,
                             int64_t batch_stride, const float* preds_2d, int64_t preds_stride, const int32_t* box_ptr_2d,
                             const float* boxes_2d, const int32_t* keep_2d, int64_t num_boxes_2d, int32_t ncam, const int32_t* box_ptr,
                             int32_t num_samples, const float* boxes, int64_t num_boxes, int64_t box_stride, int32_t box_cols,
                             const int32_t* box_labels, int32_t num_classes, int32_t code_size, float extra_height, float pos_iou_thr,
                             float min_pos_iou, bool ext, const float* old_cls_logits, int64_t logits_stride, const float* class_max_dist,
                             void* workspace, int64_t workspace_bytes, int64_t* labels, float* bbox_targets, float* bbox_weights,
                             int32_t* assigned, int32_t* source, float* stats, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (n < 0 || num_samples < 0 || num_boxes < 0 || num_boxes_2d < 0 || num_classes < 1 || xyz_stride < 3 || batch_stride < 1 ||
      preds_stride < 7 || ncam < 1 || ncam > HY_MAX_CAMS || (batch_idx_bytes != 4 && batch_idx_bytes != 8) ||
      (code_size != 8 && code_size != 10))
    return FSF_ERR_INVALID_ARG;
  if (!stats || !box_ptr || !box_ptr_2d ||
      (n > 0 && (!cluster_xyz || !batch_idx || !preds_2d || !labels || !bbox_targets || !bbox_weights || !assigned)))
    return FSF_ERR_INVALID_ARG;
  if (num_boxes > 0) {
    if (!boxes || !box_labels || (box_cols != 7 && box_cols != 9 && box_cols != 10) || box_stride < box_cols) return FSF_ERR_INVALID_ARG;
    if ((box_cols == 7) != (code_size == 8)) return FSF_ERR_INVALID_ARG;  // the coder appends box columns 7, 8 exactly when they exist
  }
  if (num_boxes_2d > 0 && (!boxes_2d || !keep_2d)) return FSF_ERR_INVALID_ARG;
  if (!(min_pos_iou > -1.f)) return FSF_ERR_INVALID_ARG;  // (-1 marks a box without a query)
  if (class_max_dist != nullptr && (logits_stride < num_classes || (n > 0 && !old_cls_logits))) return FSF_ERR_INVALID_ARG;
  if (n >= ((int64_t)1 << 24) || num_boxes >= ((int64_t)1 << 24) || num_boxes_2d >= ((int64_t)1 << 24) ||
      ((uintptr_t)boxes_2d % 16) != 0)
    return FSF_ERR_UNSUPPORTED;
  const int64_t pairs = num_boxes_2d * ncam;
  FSF_CARVE(HyLayout, l, workspace, workspace_bytes, num_boxes, pairs, n);
  if (num_boxes > 0) {
    hipLaunchKernelGGL(hybrid_box_prep_kernel, dim3((unsigned)fsf_cdiv(num_boxes, HY_BLOCK)), dim3(HY_BLOCK), 0, stream, boxes, num_boxes,
                       box_stride, extra_height, l.table, l.enc, l.box_hit);
    FSF_LAUNCH_CHECK();
  }
  const bool wide = batch_idx_bytes == 8;
  if (pairs > 0) {
    const dim3 grid((unsigned)fsf_cdiv(pairs, HY_BLOCK / FSF_WAVE));
    if (wide)
      hipLaunchKernelGGL(hybrid_gt_max_kernel<int64_t>, grid, dim3(HY_BLOCK), 0, stream, preds_2d, n, preds_stride,
                         (const int64_t*)batch_idx, batch_stride, box_ptr_2d, num_samples, boxes_2d, keep_2d, pairs, ncam, l.gt_max);
    else
      hipLaunchKernelGGL(hybrid_gt_max_kernel<int32_t>, grid, dim3(HY_BLOCK), 0, stream, preds_2d, n, preds_stride,
                         (const int32_t*)batch_idx, batch_stride, box_ptr_2d, num_samples, boxes_2d, keep_2d, pairs, ncam, l.gt_max);
    FSF_LAUNCH_CHECK();
  }
  if (l.nblk > 0) {
#define FSF_HY_LAUNCH(BT, EXT)                                                                                                          \
  hipLaunchKernelGGL((hybrid_assign_kernel<BT, EXT>), dim3((unsigned)l.nblk), dim3(HY_BLOCK), 0, stream, cluster_xyz, n, xyz_stride,     \
                     (const BT*)batch_idx, batch_stride, preds_2d, preds_stride, box_ptr_2d, boxes_2d, keep_2d, l.gt_max, num_boxes_2d,  \
                     ncam, box_ptr, num_samples, boxes, num_boxes, box_stride, box_cols, l.table, l.enc, box_labels, num_classes,          \
                     code_size, pos_iou_thr, min_pos_iou, labels, bbox_targets, bbox_weights, assigned, l.box_hit, l.partial,              \
                     old_cls_logits, logits_stride, class_max_dist, source)
    if (wide && ext) FSF_HY_LAUNCH(int64_t, true);
    else if (wide) FSF_HY_LAUNCH(int64_t, false);
    else if (ext) FSF_HY_LAUNCH(int32_t, true);
    else FSF_HY_LAUNCH(int32_t, false);
#undef FSF_HY_LAUNCH
    FSF_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(hybrid_assign_final_kernel, dim3(1), dim3(HY_BLOCK), 0, stream, l.partial, (int64_t)l.nblk, box_labels, l.box_hit, num_boxes,
                     n, l.nblk > 0, stats);
  FSF_LAUNCH_CHECK();
  return FSF_OK;
}

extern "C" int fsf_hybrid_assign(const float* cluster_xyz, int64_t n, int64_t xyz_stride, const void* batch_idx, int32_t batch_idx_bytes,
                                 int64_t batch_stride, const float* preds_2d, int64_t preds_stride, const int32_t* box_ptr_2d,
                                 const float* boxes_2d, const int32_t* keep_2d, int64_t num_boxes_2d, int32_t ncam, const int32_t* box_ptr,
                                 int32_t num_samples, const float* boxes, int64_t num_boxes, int64_t box_stride, int32_t box_cols,
                                 const int32_t* box_labels, int32_t num_classes, int32_t code_size, float extra_height, float pos_iou_thr,
                                 float min_pos_iou, void* workspace, int64_t workspace_bytes, int64_t* labels, float* bbox_targets,
                                 float* bbox_weights, int32_t* assigned, float* stats, void* stream) {
  return hybrid_assign_run(cluster_xyz, n, xyz_stride, batch_idx, batch_idx_bytes, batch_stride, preds_2d, preds_stride, box_ptr_2d,
                           boxes_2d, keep_2d, num_boxes_2d, ncam, box_ptr, num_samples, boxes, num_boxes, box_stride, box_cols, box_labels,
                           num_classes, code_size, extra_height, pos_iou_thr, min_pos_iou, false, nullptr, 0, nullptr, workspace,
                           workspace_bytes, labels, bbox_targets, bbox_weights, assigned, nullptr, stats, stream);
}

extern "C" int64_t fsf_frustum_assign_workspace_bytes(int64_t num_boxes, int64_t num_boxes_2d, int32_t ncam, int64_t n) {
  return fsf_hybrid_assign_workspace_bytes(num_boxes, num_boxes_2d, ncam, n);  // (the distance step needs no scratch of its own)
}

extern "C" int fsf_frustum_assign(const float* cluster_xyz, int64_t n, int64_t xyz_stride, const void* batch_idx, int32_t batch_idx_bytes,
                                  int64_t batch_stride, const float* preds_2d, int64_t preds_stride, const int32_t* box_ptr_2d,
                                  const float* boxes_2d, const int32_t* keep_2d, int64_t num_boxes_2d, int32_t ncam, const int32_t* box_ptr,
                                  int32_t num_samples, const float* boxes, int64_t num_boxes, int64_t box_stride, int32_t box_cols,
                                  const int32_t* box_labels, int32_t num_classes, int32_t code_size, float extra_height, float pos_iou_thr,
                                  float min_pos_iou, const float* old_cls_logits, int64_t logits_stride, const float* class_max_dist,
                                  void* workspace, int64_t workspace_bytes, int64_t* labels, float* bbox_targets, float* bbox_weights,
                                  int32_t* assigned, int32_t* source, float* stats, void* stream) {
  return hybrid_assign_run(cluster_xyz, n, xyz_stride, batch_idx, batch_idx_bytes, batch_stride, preds_2d, preds_stride, box_ptr_2d,
                           boxes_2d, keep_2d, num_boxes_2d, ncam, box_ptr, num_samples, boxes, num_boxes, box_stride, box_cols, box_labels,
                           num_classes, code_size, extra_height, pos_iou_thr, min_pos_iou, true, old_cls_logits, logits_stride,
                           class_max_dist, workspace, workspace_bytes, labels, bbox_targets, bbox_weights, assigned, source, stats, stream);
}
