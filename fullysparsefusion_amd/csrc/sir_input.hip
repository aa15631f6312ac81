// K21: the input side of a SIR layer in one pass:
//   out = cat(points / xyz_normalizer, feats, extra / extra_div) * rel_mlp(f_cluster / rel_div)
// Replaces: the per-block `torch.cat([points, out_feats], 1)` of SIR.forward (projects/mmdet3d_plugin/models/backbones/
//   sir.py:72-74; fsd_bbox_head.py:129-132 for the refine head), and in SIRLayer / DynamicClusterVFE [UNVENDORED] the
//   xyz normalisation `cat([f[:, :3] / normalizer, f[:, 3:]])`, the position MLP `rel_mlp(f_cluster / rel_dist_scaler)`
//   = 3 x (Linear(no bias) -> LayerNorm -> GELU/ReLU) built by build_mlp (ops/sst_ops.py:808-833) and the
//   `features * rel` product: two concat copies, three skinny GEMMs (K = 3|13, 16, 32: far too thin for a GEMM library),
//   three norm/act passes and a multiply — about ten launches and ~12 trips of the [n, C] activations through HBM per
//   block, twelve blocks per frame — become one read of the sources and one write of the GEMM input.
// Bytes: 4(P + Cf + Ce + R) B/row read + 4C B/row written; the position MLP runs on the fp32 matrix cores.
#include "common.h"
#include "sir_input.h"

namespace fsf {

// K21 proper: the groups strided over the grid's waves, the products stored to the [n, c] matrix in HBM, lane = channel (coalesced rows)
struct SiStoreDriver {
  static constexpr bool ALL_ROWS = false;
  float* out; int64_t out_stride; int c, lane;
  int64_t gi, gstep, groups;
  float* orow;
  __device__ __forceinline__ int64_t first() { return gi < groups ? gi : -1; }
  __device__ __forceinline__ int64_t next() { gi += gstep; return gi < groups ? gi : -1; }
  __device__ __forceinline__ void begin(int64_t row0) { orow = out + row0 * out_stride + lane; }
  __device__ __forceinline__ void put(int, int t, const float*, float v) {
    if (lane + 64 * t < c) orow[64 * t] = v;
  }
  __device__ __forceinline__ void next_row() { orow += out_stride; }
  __device__ __forceinline__ void end_group(const float*) {}
};

template <int NT3, int ACT>
__global__ void __launch_bounds__(256, 2) sir_input_kernel(SirInputArgs a) {
  extern __shared__ __attribute__((aligned(16))) char si_smem[];
  SiStoreDriver d{a.out, a.out_stride, a.c, (int)(threadIdx.x & 63), (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), (int64_t)gridDim.x * 4,
                  (a.n + 15) / 16, nullptr};
  si_run<NT3, ACT, 4>(a, si_smem, d);
}

}  // namespace fsf

using namespace fsf;

extern "C" int fsf_sir_input_gather(const float* points, int64_t points_stride, int32_t p_cols, const float xyz_normalizer[3],
                                    const float* const* feat_parts, const int64_t* feat_strides, const int32_t* feat_cols,
                                    int32_t num_parts, const int64_t* feats_index, int32_t direct_parts_mask, const float* extra,
                                    int64_t extra_stride,
                                    int32_t e_cols, float extra_div, const float* f_cluster, int64_t f_cluster_stride,
                                    int32_t r_cols, float rel_div, const float* w1, const float* g1, const float* b1, int32_t h1,
                                    const float* w2, const float* g2, const float* b2, int32_t h2, const float* w3,
                                    const float* g3, const float* b3, float eps, int32_t act, int64_t n, float* out,
                                    int64_t out_stride, void* stream_);

extern "C" int fsf_sir_input(const float* points, int64_t points_stride, int32_t p_cols, const float xyz_normalizer[3],
                             const float* feats, int64_t feats_stride, int32_t f_cols, const float* extra,
                             int64_t extra_stride, int32_t e_cols, float extra_div, const float* f_cluster,
                             int64_t f_cluster_stride, int32_t r_cols, float rel_div, const float* w1, const float* g1,
                             const float* b1, int32_t h1, const float* w2, const float* g2, const float* b2, int32_t h2,
                             const float* w3, const float* g3, const float* b3, float eps, int32_t act, int64_t n,
                             float* out, int64_t out_stride, void* stream_) {
  const float* parts[1] = {feats};
  const int64_t strides[1] = {feats_stride};
  const int32_t cols[1] = {f_cols};
  return fsf_sir_input_gather(points, points_stride, p_cols, xyz_normalizer, parts, strides, cols, f_cols > 0 ? 1 : 0, nullptr, 0, extra,
                              extra_stride, e_cols, extra_div, f_cluster, f_cluster_stride, r_cols, rel_div, w1, g1, b1, h1, w2, g2,
                              b2, h2, w3, g3, b3, eps, act, n, out, out_stride, stream_);
}

extern "C" int fsf_sir_input_gather(const float* points, int64_t points_stride, int32_t p_cols, const float xyz_normalizer[3],
                                    const float* const* feat_parts, const int64_t* feat_strides, const int32_t* feat_cols,
                                    int32_t num_parts, const int64_t* feats_index, int32_t direct_parts_mask, const float* extra,
                                    int64_t extra_stride,
                                    int32_t e_cols, float extra_div, const float* f_cluster, int64_t f_cluster_stride,
                                    int32_t r_cols, float rel_div, const float* w1, const float* g1, const float* b1, int32_t h1,
                                    const float* w2, const float* g2, const float* b2, int32_t h2, const float* w3,
                                    const float* g3, const float* b3, float eps, int32_t act, int64_t n, float* out,
                                    int64_t out_stride, void* stream_) {
  if (num_parts < 0 || num_parts > 3 || (num_parts > 0 && (!feat_parts || !feat_strides || !feat_cols))) return FSF_ERR_INVALID_ARG;
  int32_t f_cols = 0;
  for (int i = 0; i < num_parts; ++i) {
    if (feat_cols[i] < 1 || feat_strides[i] < feat_cols[i] || (n > 0 && !feat_parts[i])) return FSF_ERR_INVALID_ARG;
    if (feat_strides[i] > 0xffffffffLL) return FSF_ERR_UNSUPPORTED;  // (the gather multiplies a 32-bit row index by a 32-bit stride)
    f_cols += feat_cols[i];
  }
  const float* feats = num_parts > 0 ? feat_parts[0] : nullptr;
  const int64_t feats_stride = num_parts > 0 ? feat_strides[0] : 0;
  hipStream_t stream = (hipStream_t)stream_;
  const int c = p_cols + f_cols + e_cols;
  if (n < 0 || p_cols < 3 || f_cols < 0 || e_cols < 0 || r_cols < 1 || h1 < 1 || h2 < 1 || act < 0 || act > 2 ||
      !xyz_normalizer || !w1 || !g1 || !b1 || !w2 || !g2 || !b2 || !w3 || !g3 || !b3 ||
      (n > 0 && (!points || !f_cluster || !out || (f_cols > 0 && !feats) || (e_cols > 0 && !extra))))
    return FSF_ERR_INVALID_ARG;
  if (r_cols > SI_MAX_R || h1 > SI_MAX_H1 || h2 > SI_MAX_H2 || c > 256) return FSF_ERR_UNSUPPORTED;
  if (out_stride == 0) out_stride = c;
  if (out_stride < c || points_stride < p_cols || f_cluster_stride < r_cols) return FSF_ERR_INVALID_ARG;
  if (n == 0) return FSF_OK;
  SirInputArgs a;
  a.points = points; a.points_stride = points_stride; a.p_cols = p_cols;
  a.feats = feats; a.feats_stride = feats_stride; a.f_cols = f_cols;
  a.f0_cols = num_parts > 0 ? feat_cols[0] : 0;
  a.feats1 = num_parts > 1 ? feat_parts[1] : nullptr; a.feats1_stride = num_parts > 1 ? feat_strides[1] : 0;
  a.f1_cols = num_parts > 1 ? feat_cols[1] : 0;
  a.feats2 = num_parts > 2 ? feat_parts[2] : nullptr; a.feats2_stride = num_parts > 2 ? feat_strides[2] : 0;
  a.feats_index = num_parts > 0 ? feats_index : nullptr;
  a.direct_mask = direct_parts_mask;
  a.extra = extra; a.extra_stride = extra_stride; a.e_cols = e_cols; a.extra_div = extra_div;
  a.fcl = f_cluster; a.fcl_stride = f_cluster_stride; a.r_cols = r_cols; a.rel_div = rel_div;
  for (int i = 0; i < 3; ++i) a.norm[i] = xyz_normalizer[i];
  a.w1 = w1; a.g1 = g1; a.b1 = b1; a.h1 = h1;
  a.w2 = w2; a.g2 = g2; a.b2 = b2; a.h2 = h2;
  a.w3 = w3; a.g3 = g3; a.b3 = b3;
  a.eps = eps; a.act = act; a.out = out; a.out_stride = out_stride; a.n = n; a.c = c;
  const int64_t groups = (n + 15) / 16;
  int64_t g = (groups + 3) / 4;
  if (g > 512) g = 512;  // 2 workgroups per CU, each walks its share of the 16-row groups (the weight staging is per workgroup)
#define FSF_SI2(NT3_, ACT_)                                                                                            \
  do {                                                                                                                 \
    static std::atomic<uint64_t> attr_done{0};                                                                                      \
    FSF_HIP_TRY(fsf_set_max_dynamic_lds((const void*)sir_input_kernel<NT3_, ACT_>, (int)smem, attr_done));                                                                                                                  \
    hipLaunchKernelGGL((sir_input_kernel<NT3_, ACT_>), dim3((unsigned)g), dim3(256), smem, stream, a);                 \
  } while (0)
#define FSF_SI(NT3_)                                                                                                   \
  do {                                                                                                                 \
    constexpr size_t smem = si_smem_bytes<NT3_, 4>();                                                                  \
    if (act == 2) FSF_SI2(NT3_, 2);                                                                                    \
    else if (act == 1) FSF_SI2(NT3_, 1);                                                                               \
    else FSF_SI2(NT3_, 0);                                                                                             \
  } while (0)
  if (c <= 64) FSF_SI(4);
  else if (c <= 128) FSF_SI(8);
  else if (c <= 160) FSF_SI(10);
  else if (c <= 192) FSF_SI(12);
  else FSF_SI(16);
#undef FSF_SI
#undef FSF_SI2
  FSF_LAUNCH_CHECK();
  return FSF_OK;
}

// ----------------------------------------------------------------------------------------------------------------
// K28 (training): y = cat([points[:, :3] / normalizer, points[:, 3:], feats, extra / extra_div], 1) * h  and its adjoint.
// SIRLayer.forward (sir_layer [UNVENDORED]) in training mode: the position MLP h = rel_mlp(f_cluster / scaler) stays
// in autograd (three thin layers), but around it ATen wrote the concatenation twice (SIR.forward's cat, then the copy with the
// normalised xyz), the product, and in the backward two more products, a zero-filled slice-gradient and its accumulation:
// ~1.8 GB written per 491 k-row block.  Here the forward writes y only and the backward writes grad_h and grad_feats
// (, grad_extra) only; x is re-formed from its sources in both.  The same IEEE operations per element as the ATen chain
// (division, not multiplication by a reciprocal): bit-identical results.
namespace fsf {
struct CatMulArgs {
  const float* points; int64_t points_stride; int p_cols;
  const float* feats; int64_t feats_stride; int f_cols;
  const float* extra; int64_t extra_stride; int e_cols; float extra_div;
  float norm[3];
  const float* h;       // [n, c] contiguous
  const float* g;       // backward: grad of y [n, c] contiguous
  float* out;           // forward: y [n, c];  backward: grad_h [n, c]
  float* g_feats;       // backward (optional): [n, f_cols] contiguous
  float* g_extra;       // backward (optional): [n, e_cols] contiguous
  int64_t n; int c;
};

__device__ __forceinline__ float cm_x(const CatMulArgs& a, int64_t i, int col) {
  if (col < a.p_cols) {
    const float v = a.points[i * a.points_stride + col];
    return col < 3 ? __fdiv_rn(v, a.norm[col]) : v;
  }
  col -= a.p_cols;
  if (col < a.f_cols) return a.feats[i * a.feats_stride + col];
  col -= a.f_cols;
  return __fdiv_rn(a.extra[i * a.extra_stride + col], a.extra_div);
}

__global__ void __launch_bounds__(256) cat_mul_kernel(CatMulArgs a) {
  const int64_t total = a.n * a.c;
  const bool small = total <= 0x7fffffff;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = small ? (int64_t)((uint32_t)t / (uint32_t)a.c) : t / a.c;
    const int col = (int)(t - i * a.c);
    a.out[t] = __fmul_rn(cm_x(a, i, col), a.h[t]);
  }
}

__global__ void __launch_bounds__(256) cat_mul_bwd_kernel(CatMulArgs a) {
  const int64_t total = a.n * a.c;
  const bool small = total <= 0x7fffffff;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = small ? (int64_t)((uint32_t)t / (uint32_t)a.c) : t / a.c;
    const int col = (int)(t - i * a.c);
    const float g = a.g[t];
    a.out[t] = __fmul_rn(g, cm_x(a, i, col));  // d/dh
    const int fc = col - a.p_cols;
    if (fc >= 0) {
      const float gx = __fmul_rn(g, a.h[t]);   // d/dx
      if (fc < a.f_cols) {
        if (a.g_feats) a.g_feats[i * a.f_cols + fc] = gx;
      } else if (a.g_extra) {
        a.g_extra[i * a.e_cols + (fc - a.f_cols)] = __fdiv_rn(gx, a.extra_div);
      }
    }
  }
}
}  // namespace fsf

static int cat_mul_check(const float* points, int64_t points_stride, int32_t p_cols, const float* xyz_normalizer, const float* feats,
                         int64_t feats_stride, int32_t f_cols, const float* extra, int64_t extra_stride, int32_t e_cols, const float* h,
                         int64_t n) {
  if (n < 0 || p_cols < 3 || f_cols < 0 || e_cols < 0 || !xyz_normalizer || points_stride < p_cols || (f_cols > 0 && feats_stride < f_cols) ||
      (e_cols > 0 && extra_stride < e_cols) || (n > 0 && (!points || !h || (f_cols > 0 && !feats) || (e_cols > 0 && !extra))))
    return FSF_ERR_INVALID_ARG;
  return FSF_OK;
}

extern "C" int fsf_concat_mul(const float* points, int64_t points_stride, int32_t p_cols, const float xyz_normalizer[3], const float* feats,
                              int64_t feats_stride, int32_t f_cols, const float* extra, int64_t extra_stride, int32_t e_cols,
                              float extra_div, const float* h, int64_t n, float* out, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const int rc = cat_mul_check(points, points_stride, p_cols, xyz_normalizer, feats, feats_stride, f_cols, extra, extra_stride, e_cols, h, n);
  if (rc != FSF_OK || (n > 0 && !out)) return rc != FSF_OK ? rc : FSF_ERR_INVALID_ARG;
  if (n == 0) return FSF_OK;
  fsf::CatMulArgs a{points, points_stride, (int)p_cols, feats, feats_stride, (int)f_cols, extra, extra_stride, (int)e_cols, extra_div,
                    {xyz_normalizer[0], xyz_normalizer[1], xyz_normalizer[2]}, h, nullptr, out, nullptr, nullptr, n,
                    (int)(p_cols + f_cols + e_cols)};
  hipLaunchKernelGGL(fsf::cat_mul_kernel, dim3(fsf_stream_grid(n * a.c, 256)), dim3(256), 0, stream, a);
  FSF_LAUNCH_CHECK();
  return FSF_OK;
}

extern "C" int fsf_concat_mul_backward(const float* points, int64_t points_stride, int32_t p_cols, const float xyz_normalizer[3],
                                       const float* feats, int64_t feats_stride, int32_t f_cols, const float* extra, int64_t extra_stride,
                                       int32_t e_cols, float extra_div, const float* h, const float* grad_out, int64_t n, float* grad_h,
                                       float* grad_feats, float* grad_extra, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const int rc = cat_mul_check(points, points_stride, p_cols, xyz_normalizer, feats, feats_stride, f_cols, extra, extra_stride, e_cols, h, n);
  if (rc != FSF_OK || (n > 0 && (!grad_out || !grad_h))) return rc != FSF_OK ? rc : FSF_ERR_INVALID_ARG;
  if (n == 0) return FSF_OK;
  fsf::CatMulArgs a{points, points_stride, (int)p_cols, feats, feats_stride, (int)f_cols, extra, extra_stride, (int)e_cols, extra_div,
                    {xyz_normalizer[0], xyz_normalizer[1], xyz_normalizer[2]}, h, grad_out, grad_h, grad_feats, grad_extra, n,
                    (int)(p_cols + f_cols + e_cols)};
  hipLaunchKernelGGL(fsf::cat_mul_bwd_kernel, dim3(fsf_stream_grid(n * a.c, 256)), dim3(256), 0, stream, a);
  FSF_LAUNCH_CHECK();
  return FSF_OK;
}
