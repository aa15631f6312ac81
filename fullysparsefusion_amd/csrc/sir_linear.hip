// K21 + K22s fused: a SIR block's input side (concat, xyz normalisation, position MLP, product) and the block's first
// Linear -> LayerNorm -> GELU / ReLU -> segmented max in ONE launch; the [n, C_in] product never reaches HBM.  See include/fsf_hip.h
// (fsf_sir_input_linear_segmax) and docs/kernels/K21_K22_linear_family.md.
//
// Replaces: per SIR block, the launch pair fsf_sir_input_gather (K21, csrc/sir_input.hip) -> fsf_linear_f16w_norm_act_segmax (K22s on the f16 x 3
// path, csrc/linear_norm_act.hip): K21 wrote 4 C_in B/row that the next launch read once and nobody read again (368 MB each way per
// 510 k-row block at C_in = 180).
//
// Hand-over through LDS: K21 already parks the activated [16, C] tile of a 16-row group in a per-wave LDS slice and multiplies
// lane = channel; here the product goes back into the tile IN PLACE (columns >= C_in as zeros, what K22 makes of them), and the chunk
// loop of K22 takes its B operand — 8 k values per lane and chunk — from the tile instead of from HBM.  Both halves are the code of
// the two kernels (sir_input.h: si_run; linear_norm_act.h: the K22f scale / split, the MFMA chunk, the epilogue, the segmented max),
// the same operations on the same values in the same order: the results are bit-identical to the pair's.
//
// Shape: 8 waves x ONE 16-row group per workgroup and iteration (128 rows, as K22's 4 waves x 2 groups), one workgroup per CU = two
// waves per SIMD, K21's occupancy: the tiles (8 x 16 x (16 NT3 + 4) floats: 100 KB at NT3 = 12), K21's layer-3 fragments (24 KB) and
// K22's two weight chunks (32 KB) fill the CU's 160 KB.
#include "common.h"
#include "linear_norm_act.h"
#include "sir_input.h"

namespace fsf {

constexpr int SL_T = 8;    // 16-channel tiles of the layer (64 < c <= 128)
constexpr int SL_NW = 8;   // waves per workgroup
constexpr int SL_ROWS = FSF_SIR_FUSED_BLOCK_ROWS;
static_assert(SL_ROWS == SL_NW * 16, "one 16-row group per wave");
constexpr int SL_CHUNK_U4 = SL_T * 2 * 64;  // uint4 per weight chunk (f16 hi | lo planes)
static_assert(SL_NW * 2 == 16 && SL_CHUNK_U4 * 16 >= 16 * 128 * 4, "the segmented max parks 16 slots x 128 floats in a weight buffer");

template <int NT3>
constexpr size_t sl_smem_bytes() { return si_smem_bytes<NT3, SL_NW>() + (size_t)2 * SL_CHUNK_U4 * 16 + 384 * 4 + sizeof(LnaSegSmem); }

// the walk of si_run for the fused kernel: wave w of the workgroup takes group 8 blk + w of every 128-row block blk of the workgroup
// (a group past the last one repeats it: its rows are never stored, as in K22), keeps the products in its tile and, at the end of the
// group, runs K22's row block on it
template <int NT3, int ACT_L>
struct SlDriver {
  static constexpr bool ALL_ROWS = true;
  static constexpr int TS = NT3 * 16 + 4;
  const LnaArgs& a;
  uint4* wbuf;          // [2][SL_CHUNK_U4]
  const float* vec;     // bias | gamma | beta
  LnaSegSmem* segsm;
  const uint4* planes;  // behind the header
  int lane, wave, rowl, grp, nkc, cin;
  int64_t blk, blk_step, nblk, groups;
  int buf;
  float w_scale, w_inv;

  __device__ __forceinline__ int64_t group_of(int64_t b) const {
    const int64_t g = b * SL_NW + wave;
    return g < groups ? g : groups - 1;
  }
  __device__ __forceinline__ int64_t first() const { return blk < nblk ? group_of(blk) : -1; }
  __device__ __forceinline__ int64_t next() const { return blk + blk_step < nblk ? group_of(blk + blk_step) : -1; }
  __device__ __forceinline__ void begin(int64_t) {}
  __device__ __forceinline__ void put(int, int t, float* p, float v) {
    if (lane + 64 * t < NT3 * 16) *p = lane + 64 * t < cin ? v : 0.0f;  // (the tile row ends at 16 NT3; columns >= C_in are K22's zeros)
  }
  __device__ __forceinline__ void next_row() {}

  // weight chunk kc -> LDS buffer by LDS-DMA (fragment order in HBM == fragment order in LDS)
  __device__ __forceinline__ void stage_w(int kc, int b) {
    const float* src = reinterpret_cast<const float*>(planes + (int64_t)kc * SL_CHUNK_U4);
    float* dst = reinterpret_cast<float*>(wbuf + b * SL_CHUNK_U4);
    for (int u = wave * 64; u < SL_CHUNK_U4; u += SL_NW * 64) __builtin_amdgcn_global_load_lds(src + 4 * (u + lane), dst + 4 * u, 16, 0, 0);
  }

  // K22's row block (XM = 2, SEG, LayerNorm, no addend) with the x chunks read from the wave's tile
  __device__ __forceinline__ void end_group(const float* tile) {
    const int64_t row0 = blk * SL_ROWS + (int64_t)wave * 16;
    LnaSegBlockT<1> sb;
    {
      const int64_t r = row0 + rowl;
      sb.sid[0] = (int)a.seg_ids[r < a.n ? r : a.n - 1];
      sb.sid_before = row0 > 0 ? (int)a.seg_ids[row0 - 1 < a.n ? row0 - 1 : a.n - 1] : -1;
      sb.sid_after = row0 + 16 < a.n ? (int)a.seg_ids[row0 + 16] : -1;
    }
    lna_f32x4 acc[1][SL_T];
#pragma unroll
    for (int t = 0; t < SL_T; ++t) acc[0][t] = lna_f32x4{0.f, 0.f, 0.f, 0.f};
    float xinv[1], xs_cur[1];
    const float* xrow = tile + rowl * TS + 8 * grp;  // this lane's 8 k values of chunk kc: xrow + 32 kc (16-byte aligned)
    for (int kc = 0; kc < nkc; ++kc, buf ^= 1) {
      float xc[1][8];
      const float4 p = *reinterpret_cast<const float4*>(xrow + kc * LNA_KC), q = *reinterpret_cast<const float4*>(xrow + kc * LNA_KC + 4);
      xc[0][0] = p.x; xc[0][1] = p.y; xc[0][2] = p.z; xc[0][3] = p.w;
      xc[0][4] = q.x; xc[0][5] = q.y; xc[0][6] = q.z; xc[0][7] = q.w;
      lna_u32x4 xh[1], xl[1];
      lna_xf_scale_split<1, SL_T>(xc, kc, xs_cur, xinv, xh, xl, acc, w_scale, 0x1p126f, 0x1p-126f, false);
      // this chunk's weights (DMA issued one chunk ago) have landed, and every wave is done reading the other buffer
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      if (kc + 1 < nkc) stage_w(kc + 1, buf ^ 1);
      else if (blk + blk_step < nblk) stage_w(0, buf ^ 1);  // first chunk of the next row block: lands under the epilogue and the next MLP
      lna_mfma_f16_chunk<1, SL_T>(wbuf + buf * SL_CHUNK_U4, lane, xh, xl, acc);
    }
    {  // back to the unscaled product: both scales are powers of two (exact)
      const float sc = xinv[0] * w_inv;
#pragma unroll
      for (int t = 0; t < SL_T; ++t) acc[0][t] = acc[0][t] * sc;
    }
    float* slots = reinterpret_cast<float*>(wbuf + (buf ^ 1) * SL_CHUNK_U4);  // (the chunk loop's last buffer, free now)
    sb.blk_row0 = blk * SL_ROWS; sb.wave = wave; sb.slots = slots; sb.sm = segsm;
    __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): this wave's LDS reads of the last chunk have returned ...
    __builtin_amdgcn_s_barrier();        // ... and so have every other wave's: the slots may overlay that buffer
    if (lane < 2) segsm->slot_sid[2 * wave + lane] = -1;
    lna_epilogue<SL_T, true, 1, ACT_L, 1>(a, acc, row0, 0, rowl, grp, vec, &sb);
    lna_seg_merge(a, slots, segsm);
    blk += blk_step;
  }
};

template <int NT3, int ACT>  // ACT: the activation of the position MLP and of the layer (1 ReLU / 2 GELU)
__global__ void __launch_bounds__(SL_NW * 64, 1) sir_linear_kernel(SirInputArgs si, LnaArgs a) {
  extern __shared__ __attribute__((aligned(16))) char sl_smem[];
  char* si_smem = sl_smem;  // K21's part first: its tiles are read up to one row stride past their columns, never past the allocation
  uint4* wbuf = reinterpret_cast<uint4*>(sl_smem + si_smem_bytes<NT3, SL_NW>());
  float* vec = reinterpret_cast<float*>(wbuf + 2 * SL_CHUNK_U4);
  LnaSegSmem* segsm = reinterpret_cast<LnaSegSmem*>(vec + 384);
  if (reinterpret_cast<const unsigned*>(a.planes)[FMT_HDR_TAG] != LNA_F16_TAG)
    __builtin_trap();  // a buffer that fsf_linear_prepare_weight_f16 did not write: the launch fails loudly instead of multiplying garbage
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  SlDriver<NT3, ACT> d{a, wbuf, vec, segsm, a.planes + FMT_HDR_U4, lane, wave, lane & 15, lane >> 4, (a.k + LNA_KC - 1) / LNA_KC, a.k,
                       (int64_t)blockIdx.x, (int64_t)gridDim.x, (a.n + SL_ROWS - 1) / SL_ROWS, (a.n + 15) / 16, 0,
                       reinterpret_cast<const float*>(a.planes)[FMT_HDR_SCALE], reinterpret_cast<const float*>(a.planes)[FMT_HDR_INV_SCALE]};
  lna_stage_vectors(a, 0, vec);
  d.stage_w(0, 0);
  si_run<NT3, ACT, SL_NW>(si, si_smem, d);
}

}  // namespace fsf

using namespace fsf;

extern "C" int fsf_sir_input_linear_segmax(const float* points, int64_t points_stride, int32_t p_cols, const float xyz_normalizer[3],
                                           const float* const* feat_parts, const int64_t* feat_strides, const int32_t* feat_cols,
                                           int32_t num_parts, const int64_t* feats_index, int32_t direct_parts_mask, const float* extra,
                                           int64_t extra_stride, int32_t e_cols, float extra_div, const float* f_cluster,
                                           int64_t f_cluster_stride, int32_t r_cols, float rel_div, const float* w1, const float* g1,
                                           const float* b1, int32_t h1, const float* w2, const float* g2, const float* b2, int32_t h2,
                                           const float* w3, const float* g3, const float* b3, float mlp_eps, int32_t mlp_act, int64_t n,
                                           const void* w_planes, int32_t c, const float* bias, int32_t norm, const float* gamma,
                                           const float* beta, float eps, int32_t act, const int64_t* seg_ids, int64_t num_segments,
                                           float* seg_out, int64_t seg_out_stride, float* out, int64_t out_stride, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  // ---- K21's side (fsf_sir_input_gather)
  if (num_parts < 0 || num_parts > 3 || (num_parts > 0 && (!feat_parts || !feat_strides || !feat_cols))) return FSF_ERR_INVALID_ARG;
  int32_t f_cols = 0;
  for (int i = 0; i < num_parts; ++i) {
    if (feat_cols[i] < 1 || feat_strides[i] < feat_cols[i] || (n > 0 && !feat_parts[i])) return FSF_ERR_INVALID_ARG;
    if (feat_strides[i] > 0xffffffffLL) return FSF_ERR_UNSUPPORTED;  // (the gather multiplies a 32-bit row index by a 32-bit stride)
    f_cols += feat_cols[i];
  }
  const int cin = p_cols + f_cols + e_cols;
  if (n < 0 || p_cols < 3 || e_cols < 0 || r_cols < 1 || h1 < 1 || h2 < 1 || mlp_act < 0 || mlp_act > 2 || !xyz_normalizer || !w1 || !g1 ||
      !b1 || !w2 || !g2 || !b2 || !w3 || !g3 || !b3 || (n > 0 && (!points || !f_cluster || (e_cols > 0 && !extra))))
    return FSF_ERR_INVALID_ARG;
  if (points_stride < p_cols || f_cluster_stride < r_cols || (e_cols > 0 && extra_stride < e_cols)) return FSF_ERR_INVALID_ARG;
  // ---- K22s's side (fsf_linear_f16w_norm_act_segmax without a per-row addend)
  if (c < 1 || !w_planes || norm < 0 || norm > 2 || act < 0 || act > 2 || (norm != 0 && (!gamma || !beta)) || num_segments < 0 ||
      (n > 0 && (!seg_ids || !seg_out || num_segments < 1)))
    return FSF_ERR_INVALID_ARG;
  if (out && out_stride < c) return FSF_ERR_INVALID_ARG;
  // ---- the fused kernel's scope: the SIR blocks' first layers as the frame runs them; the caller runs the two kernels for the rest
  if (r_cols > SI_MAX_R || h1 > SI_MAX_H1 || h2 > SI_MAX_H2 || cin <= 128 || cin > 192) return FSF_ERR_UNSUPPORTED;
  if (norm != 1 || (act != 1 && act != 2) || mlp_act != act || c <= 64 || c > 128 || (c % 4) != 0 || ((uintptr_t)w_planes % 16) != 0 ||
      (seg_out_stride % 4) != 0 || seg_out_stride < c || ((uintptr_t)seg_out % 16) != 0 ||
      (out && ((out_stride % 4) != 0 || ((uintptr_t)out % 16) != 0)) || n >= ((int64_t)1 << 31) || num_segments >= LNA_SLOT_HEAD_OPEN ||
      num_segments * seg_out_stride >= ((int64_t)1 << 31))
    return FSF_ERR_UNSUPPORTED;
  if (n == 0) return FSF_OK;
  SirInputArgs s;
  s.points = points; s.points_stride = points_stride; s.p_cols = p_cols;
  s.feats = num_parts > 0 ? feat_parts[0] : nullptr; s.feats_stride = num_parts > 0 ? feat_strides[0] : 0; s.f_cols = f_cols;
  s.f0_cols = num_parts > 0 ? feat_cols[0] : 0;
  s.feats1 = num_parts > 1 ? feat_parts[1] : nullptr; s.feats1_stride = num_parts > 1 ? feat_strides[1] : 0;
  s.f1_cols = num_parts > 1 ? feat_cols[1] : 0;
  s.feats2 = num_parts > 2 ? feat_parts[2] : nullptr; s.feats2_stride = num_parts > 2 ? feat_strides[2] : 0;
  s.feats_index = num_parts > 0 ? feats_index : nullptr;
  s.direct_mask = direct_parts_mask;
  s.extra = extra; s.extra_stride = extra_stride; s.e_cols = e_cols; s.extra_div = extra_div;
  s.fcl = f_cluster; s.fcl_stride = f_cluster_stride; s.r_cols = r_cols; s.rel_div = rel_div;
  for (int i = 0; i < 3; ++i) s.norm[i] = xyz_normalizer[i];
  s.w1 = w1; s.g1 = g1; s.b1 = b1; s.h1 = h1;
  s.w2 = w2; s.g2 = g2; s.b2 = b2; s.h2 = h2;
  s.w3 = w3; s.g3 = g3; s.b3 = b3;
  s.eps = mlp_eps; s.act = mlp_act; s.out = nullptr; s.out_stride = 0; s.n = n; s.c = cin;
  LnaArgs a{nullptr, 0, cin, (const uint4*)w_planes, bias, gamma, beta, eps, (int)norm, (int)act, out, out_stride, n, (int)c,
            nullptr, nullptr, 0, 128, (int)c, 0, seg_ids, seg_out, seg_out_stride, nullptr};
  const int64_t nblk = (n + SL_ROWS - 1) / SL_ROWS;
  const unsigned g = (unsigned)(nblk < 256 ? nblk : 256);  // one workgroup per CU, each walks its share of the 128-row blocks
#define FSF_SL(NT3_, ACT_)                                                                                                  \
  do {                                                                                                                      \
    constexpr size_t smem = sl_smem_bytes<NT3_>();                                                                          \
    static std::atomic<uint64_t> attr_done{0};                                                                              \
    FSF_HIP_TRY(fsf_set_max_dynamic_lds((const void*)sir_linear_kernel<NT3_, ACT_>, (int)smem, attr_done));                 \
    hipLaunchKernelGGL((sir_linear_kernel<NT3_, ACT_>), dim3(g), dim3(SL_NW * 64), smem, stream, s, a);                     \
  } while (0)
  if (cin <= 160) {
    if (act == 2) FSF_SL(10, 2);
    else FSF_SL(10, 1);
  } else {
    if (act == 2) FSF_SL(12, 2);
    else FSF_SL(12, 1);
  }
#undef FSF_SL
  FSF_LAUNCH_CHECK();
  return FSF_OK;
}
