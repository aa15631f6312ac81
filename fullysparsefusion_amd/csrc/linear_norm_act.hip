// K22: per-point Linear (+ bias) -> LayerNorm | eval-BatchNorm affine -> ReLU | GELU in one pass, fp32 in / fp32 out.
// See include/fsf_hip.h.
//
// Replaces (inference): the [Linear, norm, act] blocks that build_mlp (projects/mmdet3d_plugin/ops/sst_ops.py:808-833) and
// DynamicVFELayer [UNVENDORED] put on every point: a dense fp32 GEMM on the library (70 % of the fp32 matrix-pipe peak
// at best) + one more pass over the [n, C] activations for norm + act.
//
// The fp32 matrix pipe (v_mfma_f32_16x16x4_f32, 157 TFLOP/s) is 1/16 of the bf16 one, so the product is formed on
// v_mfma_f32_16x16x32_bf16 from an EXACT three-way split of both operands: x = hi + mid + lo with hi = x truncated to
// its top 8 significant bits (a bf16), mid = the same of x - hi, lo = x - hi - mid (8 bits left: a bf16, exactly) —
// three 8-bit pieces cover the 24-bit fp32 significand, nothing is rounded away.  a*b is then the sum of nine bf16
// products (each exact in the fp32 accumulator's input); the six leading ones are issued, the dropped mid*lo, lo*mid,
// lo*lo terms are < 2^-23 of |a*b| together — the size of ONE fp32 rounding — and the accumulation is fp32 as on the
// fp32 pipe.  6 x ~17 cycles per 16x16x32 block instead of 8 x 32: the matrix phase is 2.5x shorter at fp32 accuracy
// (tests: error vs float64 no larger than torch's fp32 F.linear).  This is not a reduced-precision mode.
//
// Transposed formulation (as K21): out^T[channel, row] = W[channel, k] x X^T[k, row]; the weights are the A operand
// (pre-split once per layer into fragment-ordered bf16 planes by fsf_linear_prepare_weight, streamed through LDS in
// 64-wide k chunks, double-buffered by LDS-DMA), 16 point rows are the B operand (loaded straight from HBM in operand
// layout — lane (row, g) reads 32 contiguous bytes per k step — and split in registers).  A lane ends up with channels
// 16 t + 4 g + r of its row: LayerNorm is an in-lane sum + two shuffles, the result leaves as 16-byte stores.
#include <stdlib.h>
#include <algorithm>

#include "common.h"
#include "linear_norm_act.h"

namespace fsf {

// weight [c, k] fp32 -> fragment-ordered bf16 planes (zero padded to T tiles x KP)
__global__ void __launch_bounds__(256)
    lna_prepare_kernel(const float* __restrict__ w, int k, int c, int T, int nkc, int nslice, int slice_w, uint4* planes) {
  const int64_t total = (int64_t)nslice * nkc * T * 64;  // (slice, chunk, tile, lane): three 16-byte fragments each
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int lane = (int)(idx & 63);
    const int t = (int)((idx >> 6) % T);
    const int kc = (int)(((idx >> 6) / T) % nkc);
    const int slice = (int)((idx >> 6) / ((int64_t)T * nkc));
    const int lc = 16 * t + (lane & 15), col = slice_w * slice + lc, k0 = kc * LNA_KC + 8 * (lane >> 4);
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = (lc < slice_w && col < c && k0 + e < k) ? w[(int64_t)col * k + k0 + e] : 0.0f;
    lna_u32x4 hi, mid, lo;
    fmt_split_bf16(v, hi, mid, lo);
    uint4* dst = planes + (((int64_t)slice * nkc + kc) * T + t) * 3 * 64 + lane;
    dst[0] = make_uint4(hi[0], hi[1], hi[2], hi[3]);
    dst[64] = make_uint4(mid[0], mid[1], mid[2], mid[3]);
    dst[128] = make_uint4(lo[0], lo[1], lo[2], lo[3]);
  }
}

// weight [c, k] fp32 -> header (inverse scale, scale, max |w| bits: already there, fsf_weight_layer_absmax) + fragment-ordered f16
// hi | lo planes of W * s_w
__global__ void __launch_bounds__(256)
    lna_prepare_f16_kernel(const float* __restrict__ w, int k, int c, int T, int nkc, int nslice, int slice_w, float* __restrict__ hdr,
                           uint4* __restrict__ planes) {
  float s_w, inv_w;
  fmt_pick_scale(__uint_as_float(reinterpret_cast<const unsigned*>(hdr)[FMT_HDR_AMAX_BITS]), s_w, inv_w);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    hdr[FMT_HDR_INV_SCALE] = inv_w;
    hdr[FMT_HDR_SCALE] = s_w;
    reinterpret_cast<unsigned*>(hdr)[FMT_HDR_TAG] = LNA_F16_TAG;  // the format's tag word: the f16-weight kernels refuse a buffer without it
  }
  const int64_t total = (int64_t)nslice * nkc * T * 64;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int lane = (int)(idx & 63);
    const int t = (int)((idx >> 6) % T);
    const int kc = (int)(((idx >> 6) / T) % nkc);
    const int slice = (int)((idx >> 6) / ((int64_t)T * nkc));
    const int lc = 16 * t + (lane & 15), col = slice_w * slice + lc, k0 = kc * LNA_KC + 8 * (lane >> 4);
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = (lc < slice_w && col < c && k0 + e < k) ? w[(int64_t)col * k + k0 + e] : 0.0f;
    lna_u32x4 hi, lo;
    fmt_split_f16(v, s_w, hi, lo);
    uint4* dst = planes + (((int64_t)slice * nkc + kc) * T + t) * 2 * 64 + lane;
    dst[0] = make_uint4(hi[0], hi[1], hi[2], hi[3]);
    dst[64] = make_uint4(lo[0], lo[1], lo[2], lo[3]);
  }
}

// fp32 rows [n, c] (optionally through LayerNorm + ReLU / GELU first: the norm pass that follows a Linear wider than 128 channels)
// -> row planes [n][c / 8][2][8] f16 + one inverse scale per row (+ the fp32 rows themselves when `out` is given).  One wave per row;
// lane l owns the 8-channel blocks l, l + 64, ... (BL of them: c <= 512 BL).
template <int BL, int NORM, int ACT>
__global__ void __launch_bounds__(256)
    rows_to_planes_kernel(const float* __restrict__ x, int64_t n, int c, int64_t x_stride, const float* __restrict__ gamma,
                          const float* __restrict__ beta, float eps, uint4* __restrict__ planes, float* __restrict__ inv_scales,
                          float* __restrict__ out, int64_t out_stride) {
  const int lane = threadIdx.x & 63;
  const int nb = c >> 3;
  const float inv_c = 1.0f / (float)c;
  for (int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); row < n; row += (int64_t)gridDim.x * 4) {
    float v[BL][8];
#pragma unroll
    for (int b = 0; b < BL; ++b) {
      const int blk = lane + 64 * b;
      if (blk < nb) {
        const float4 p = *reinterpret_cast<const float4*>(x + row * x_stride + 8 * blk);
        const float4 q = *reinterpret_cast<const float4*>(x + row * x_stride + 8 * blk + 4);
        v[b][0] = p.x; v[b][1] = p.y; v[b][2] = p.z; v[b][3] = p.w; v[b][4] = q.x; v[b][5] = q.y; v[b][6] = q.z; v[b][7] = q.w;
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[b][e] = 0.0f;
      }
    }
    if (NORM == 1) {
      float s = 0.0f;
#pragma unroll
      for (int b = 0; b < BL; ++b)
#pragma unroll
        for (int e = 0; e < 8; ++e) s += v[b][e];
      const float mean = fsf_wave_sum(s) * inv_c;
      float q = 0.0f;
#pragma unroll
      for (int b = 0; b < BL; ++b)
        if (lane + 64 * b < nb) {
#pragma unroll
          for (int e = 0; e < 8; ++e) { const float d = v[b][e] - mean; q = fmaf(d, d, q); }
        }
      const float rstd = rsqrtf(fsf_wave_sum(q) * inv_c + eps);
#pragma unroll
      for (int b = 0; b < BL; ++b) {
        const int blk = lane + 64 * b;
        if (blk < nb) {
          const float4 g0 = *reinterpret_cast<const float4*>(gamma + 8 * blk), g1 = *reinterpret_cast<const float4*>(gamma + 8 * blk + 4);
          const float4 b0 = *reinterpret_cast<const float4*>(beta + 8 * blk), b1 = *reinterpret_cast<const float4*>(beta + 8 * blk + 4);
          const float gg[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w}, bb[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
          for (int e = 0; e < 8; e += 2) {
            lna_f32x2 y = (lna_f32x2{v[b][e], v[b][e + 1]} - lna_pk(mean)) * lna_pk(rstd) * lna_f32x2{gg[e], gg[e + 1]} + lna_f32x2{bb[e], bb[e + 1]};
            y = lna_act2(y, ACT);
            v[b][e] = y.x; v[b][e + 1] = y.y;
          }
        }
      }
    } else if (ACT != 0) {
#pragma unroll
      for (int b = 0; b < BL; ++b)
#pragma unroll
        for (int e = 0; e < 8; e += 2) {
          const lna_f32x2 y = lna_act2(lna_f32x2{v[b][e], v[b][e + 1]}, ACT);
          v[b][e] = y.x; v[b][e + 1] = y.y;
        }
    }
    float amax = 0.0f;
#pragma unroll
    for (int b = 0; b < BL; ++b)
#pragma unroll
      for (int e = 0; e < 8; ++e) amax = fmaxf(amax, fabsf(v[b][e]));
    amax = fsf_wave_max(amax);
    float s_row, inv_row;
    fmt_pick_scale(amax, s_row, inv_row);
    if (lane == 0) inv_scales[row] = inv_row;
#pragma unroll
    for (int b = 0; b < BL; ++b) {
      const int blk = lane + 64 * b;
      if (blk < nb) {
        lna_u32x4 hi, lo;
        fmt_split_f16(v[b], s_row, hi, lo);
        uint4* dst = planes + (row * nb + blk) * 2;
        dst[0] = make_uint4(hi[0], hi[1], hi[2], hi[3]);
        dst[1] = make_uint4(lo[0], lo[1], lo[2], lo[3]);
        if (out) {
          *reinterpret_cast<float4*>(out + row * out_stride + 8 * blk) = make_float4(v[b][0], v[b][1], v[b][2], v[b][3]);
          *reinterpret_cast<float4*>(out + row * out_stride + 8 * blk + 4) = make_float4(v[b][4], v[b][5], v[b][6], v[b][7]);
        }
      }
    }
  }
}


// LNA_NW = 4 waves per workgroup.  A weight chunk enters the CU once per WORKGROUP and chunk (LDS-DMA), so three 4-wave workgroups per
// CU take the same 24 KB in three times per 128 rows each; ONE 12-wave workgroup per CU (same 12 waves, same registers) would take it in
// once per 384 rows.  Measured (round 3, same box): no faster in isolation (510 k x 256 -> 128: 277 vs 279 us; k = 128 .. 180: 5-15 %
// SLOWER — a barrier over twelve waves per chunk) and 7 % slower in the frame (a 768-thread workgroup shuts the other stream's kernels
// out of its CU) — so the weight stream is not what this kernel waits for, and the 12-wave form is gone (profiles/r3_k22_ablations.txt).
template <int T, bool SEG = false, int NORM_CT = -1, int ACT_CT = -1, int XM = 0>  // 16-channel tiles (c <= 16 T); SEG: +
// segmented max of the output (rows sorted by segment), norm / act fixed at compile time; XM = 1 (XP): x and W arrive as f16 hi | lo
// planes (K22h); XM = 2 (XF, K22f): fp32 x split IN the kernel into f16 hi | lo of x * s_row (s_row: the running power-of-two unit of the
// row, below), W as f16 planes — three MFMA passes per product instead of the six of the exact bf16 split (XM = 0)
__global__ void __launch_bounds__(LNA_NW * 64, SEG ? LNA_SEG_WPS : LNA_WPS) linear_norm_act_kernel(LnaArgs a) {
  constexpr bool XP = XM == 1, XF = XM == 2;
  constexpr int NPL = XM != 0 ? 2 : 3;        // weight planes per tile
  constexpr int CHUNK_U4 = T * NPL * 64;      // uint4 per weight chunk
  static_assert(!SEG || (LNA_NW == 4 && CHUNK_U4 * 16 >= 16 * 128 * 4), "the segmented max parks 16 x 128 floats in a weight buffer");
  extern __shared__ __attribute__((aligned(16))) char lna_smem[];
  uint4* wbuf = reinterpret_cast<uint4*>(lna_smem);  // [2][CHUNK_U4], then 384 floats of per-channel vectors (, then LnaSegSmem)
  float* vec = reinterpret_cast<float*>(wbuf + 2 * CHUNK_U4);
  LnaSegSmem* segsm = reinterpret_cast<LnaSegSmem*>(vec + 384);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int rowl = lane & 15, grp = lane >> 4;
  const int nkc = (a.k + LNA_KC - 1) / LNA_KC;
  const int64_t nblk = (a.n + LNA_ROWS - 1) / LNA_ROWS;
  // more than 128 output channels: gridDim.y slices of 128, each an independent [rows, 128] product (no LayerNorm then:
  // its statistics span the slices; the caller runs fsf_norm_act on the result)
  // XP launches come as a 1-D grid laid out so that the workgroups that share a row block (one per 128-channel slice) have the same
  // id modulo 8, i.e. land on the same XCD and meet their x rows in its L2: id = xcd + 8 (slice + nslice j), row-block lane 8 j + xcd
  int slice_id = (int)blockIdx.y;
  int64_t blk_first = blockIdx.x, blk_step = gridDim.x;
  if constexpr (XP) {
    const int nslice = (a.c + a.slice_w - 1) / a.slice_w;
    const int wg = (int)blockIdx.x, q = wg >> 3;
    slice_id = q % nslice;
    blk_first = (int64_t)(q / nslice) * 8 + (wg & 7);
    blk_step = gridDim.x / nslice;
  }
  const int ch_base = a.slice_w * slice_id;
  const uint4* planes = a.planes + (XM != 0 ? FMT_HDR_U4 : 0) + (int64_t)slice_id * nkc * CHUNK_U4;  // (f16 planes: behind the 256-byte header)
  if (XM != 0 && reinterpret_cast<const unsigned*>(a.planes)[FMT_HDR_TAG] != LNA_F16_TAG)
    __builtin_trap();  // a buffer that fsf_linear_prepare_weight_f16 did not write: the launch fails loudly instead of multiplying garbage

  // weight chunk kc -> LDS buffer by LDS-DMA: fragment order in HBM == fragment order in LDS, 1 KB per wave instruction
  auto stage_w = [&](int kc, int buf) {
    const float* src = reinterpret_cast<const float*>(planes + (int64_t)kc * CHUNK_U4);
    float* dst = reinterpret_cast<float*>(wbuf + buf * CHUNK_U4);
    for (int u = wave * 64; u < CHUNK_U4; u += LNA_NW * 64)
      __builtin_amdgcn_global_load_lds(src + 4 * (u + lane), dst + 4 * u, 16, 0, 0);
  };

  // The (row block, k chunk) sequence of a workgroup is ONE software pipeline: during the last chunk of a block the first
  // weight chunk and the first x chunk of the NEXT block are already requested, so the epilogue (norm, activation,
  // stores) runs with them in flight instead of every block starting with an exposed HBM round trip.
  const float* xrow[LNA_RG];
  auto set_rows = [&](int64_t blk) {
#pragma unroll
    for (int rg = 0; rg < LNA_RG; ++rg) {
      int64_t r = blk * LNA_ROWS + (int64_t)wave * (LNA_RG * 16) + 16 * rg + rowl;
      if (r >= a.n) r = a.n - 1;  // rows past n repeat the last one (finite, never stored)
      if constexpr (XP) xrow[rg] = a.x + r * (int64_t)a.k;  // (plane rows: k / 8 blocks x 2 planes x 16 B = 4 k bytes, like fp32 rows)
      else xrow[rg] = a.x + r * a.x_stride + (int64_t)slice_id * a.x_slice_off;
    }
  };
  // raw x of one chunk: [row group][8 floats]; the NEXT chunk is requested while this one is split and multiplied.
  // Always exactly two 16-byte loads per row group: offsets past the row are clamped into it (x_stride is a multiple
  // of 4 and >= k, so a quad that holds any column < k is never clamped) and the columns >= k are zeroed afterwards
  // (what follows the row in memory may be NaN).
  const int last_quad = XP ? 0 : (int)a.x_stride - 4 - (int)((int64_t)slice_id * a.x_slice_off);  // (relative to this slice's first column)
  auto load_x = [&](int kc, float (&v)[LNA_RG][8]) {
#pragma unroll
    for (int rg = 0; rg < LNA_RG; ++rg) {
      if constexpr (XP) {  // k block 4 kc + grp of the row: hi plane | lo plane, 32 contiguous bytes (k is a multiple of 32 here)
        const float4* pb = reinterpret_cast<const float4*>(xrow[rg]) + 2 * (4 * kc + grp);
        const float4 p = pb[0], q = pb[1];
        v[rg][0] = p.x; v[rg][1] = p.y; v[rg][2] = p.z; v[rg][3] = p.w;
        v[rg][4] = q.x; v[rg][5] = q.y; v[rg][6] = q.z; v[rg][7] = q.w;
        continue;
      }
      const int kq = kc * LNA_KC + 8 * grp;  // this lane's 8 k values
      const float4 p = *reinterpret_cast<const float4*>(xrow[rg] + min(kq, last_quad));
      const float4 q = *reinterpret_cast<const float4*>(xrow[rg] + min(kq + 4, last_quad));
      v[rg][0] = p.x; v[rg][1] = p.y; v[rg][2] = p.z; v[rg][3] = p.w;
      v[rg][4] = q.x; v[rg][5] = q.y; v[rg][6] = q.z; v[rg][7] = q.w;
    }
  };
  lna_stage_vectors(a, ch_base, vec);
  // (XF) the weight scale s_w, and the cap of a row's FIRST scale: with a per-row addend in the accumulators — it enters them multiplied
  // by s * s_w — s * s_w stays <= 2^40 (an addend below 2^87 cannot overflow; a row whose values all lie below 2^-27 / s_w loses bits
  // it could not contribute next to an addend anyway); without one, any scale a finite row asks for
  float w_scale = 1.0f, xs_cap = 0x1p126f, xs_cap_inv = 0x1p-126f;
  if constexpr (XF) {
    w_scale = reinterpret_cast<const float*>(a.planes)[FMT_HDR_SCALE];
    if (a.row_add) {
      int e = (int)((__float_as_uint(reinterpret_cast<const float*>(a.planes)[FMT_HDR_INV_SCALE]) >> 23) & 0xffu) - 127 + 40;
      e = e < -126 ? -126 : (e > 126 ? 126 : e);
      xs_cap = __uint_as_float((unsigned)(e + 127) << 23);
      xs_cap_inv = __uint_as_float((unsigned)(127 - e) << 23);
    }
  }
  // The per-row addend (`cat([point, group[inv]]) W^T` = point W_left^T + (group W_right^T)[inv]) enters through the ACCUMULATORS: they
  // start a row block as the gathered addend rows instead of zeros, the MFMAs accumulate on top.  In the epilogue (round 4) the gather
  // was four exposed round trips per block — index, then 4 + 4 tiles per row group, twice — 20 % of the grouped K22s kernel
  // (profiles/r5_lna_timeline.txt); now the index of the NEXT block's rows is fetched under the chunk loop and the 16 row loads of a
  // block are in flight together, into registers that are free at that point, behind the first chunk's split.
  int64_t radd_idx[LNA_RG];
  auto fetch_addend_index = [&](int64_t blk) {
    if (a.row_add) {
#pragma unroll
      for (int rg = 0; rg < LNA_RG; ++rg) {
        const int64_t r = blk * LNA_ROWS + (int64_t)wave * (LNA_RG * 16) + 16 * rg + rowl;
        radd_idx[rg] = a.row_add_index[r < a.n ? r : a.n - 1];
      }
    }
  };
  LnaArgs a_epi = a;  // (the epilogue's copy: the addend is already in the accumulators)
  a_epi.row_add = nullptr;
  float xc[LNA_RG][8];
  int buf = 0;
  if (blk_first < nblk) {
    fetch_addend_index(blk_first);
    set_rows(blk_first);
    load_x(0, xc);
    stage_w(0, 0);
  }
  for (int64_t blk = blk_first; blk < nblk; blk += blk_step) {
    const int64_t row0 = blk * LNA_ROWS + (int64_t)wave * (LNA_RG * 16);
    LnaSegBlock sb;
    if constexpr (SEG) {  // the rows' segment ids (and those of the rows just above / below the wave's 32) arrive under the chunk loop
#pragma unroll
      for (int rg = 0; rg < LNA_RG; ++rg) {
        const int64_t r = row0 + 16 * rg + rowl;
        sb.sid[rg] = (int)a.seg_ids[r < a.n ? r : a.n - 1];
      }
      sb.sid_before = row0 > 0 ? (int)a.seg_ids[row0 - 1 < a.n ? row0 - 1 : a.n - 1] : -1;
      sb.sid_after = row0 + 16 * LNA_RG < a.n ? (int)a.seg_ids[row0 + 16 * LNA_RG] : -1;
    }
    lna_f32x4 acc[LNA_RG][T];
#pragma unroll
    for (int rg = 0; rg < LNA_RG; ++rg)
#pragma unroll
      for (int t = 0; t < T; ++t) acc[rg][t] = lna_f32x4{0.f, 0.f, 0.f, 0.f};
    if (a.row_add) {
#pragma unroll
      for (int rg = 0; rg < LNA_RG; ++rg) {
        const float* add = a.row_add + radd_idx[rg] * a.row_add_stride;
#pragma unroll
        for (int t = 0; t < T; ++t) {
          const int lc0 = 16 * t + 4 * grp, ch0 = ch_base + lc0;
          if (lc0 < a.slice_w && ch0 < a.c) {
            const float4 b = *reinterpret_cast<const float4*>(add + ch0);
            acc[rg][t] = lna_f32x4{b.x, b.y, b.z, b.w};
          }
        }
      }
    }
    float xinv[LNA_RG];
    float xs_cur[LNA_RG];  // (XF) the unit the row's accumulators are kept in: acc = (true sum) * xs_cur * s_w; xinv = 1 / xs_cur
    if constexpr (XP) {  // the rows' inverse scales (requested here, used after the chunk loop)
#pragma unroll
      for (int rg = 0; rg < LNA_RG; ++rg) {
        const int64_t r = row0 + 16 * rg + rowl;
        xinv[rg] = a.x_inv_scale[r < a.n ? r : a.n - 1];
      }
    }
    for (int kc = 0; kc < nkc; ++kc, buf ^= 1) {
      // split the chunk that arrived while the previous one was multiplied; its registers then take the next prefetch
      lna_u32x4 xh[LNA_RG], xm[LNA_RG], xl[LNA_RG];
      if constexpr (XP) {  // the planes ARE the operands: nothing to split
#pragma unroll
        for (int rg = 0; rg < LNA_RG; ++rg) {
#pragma unroll
          for (int e = 0; e < 4; ++e) { xh[rg][e] = __float_as_uint(xc[rg][e]); xl[rg][e] = __float_as_uint(xc[rg][4 + e]); }
          xm[rg] = xh[rg];
        }
      } else
      if ((kc + 1) * LNA_KC > a.k) {  // (uniform: the last chunk of a k that is not a multiple of 32)
#pragma unroll
        for (int rg = 0; rg < LNA_RG; ++rg)
#pragma unroll
          for (int e = 0; e < 8; ++e)
            if (kc * LNA_KC + 8 * grp + e >= a.k) xc[rg][e] = 0.0f;
      }
      if constexpr (XM == 0) {
#pragma unroll
        for (int rg = 0; rg < LNA_RG; ++rg) fmt_split_bf16(xc[rg], xh[rg], xm[rg], xl[rg]);
      }
      if constexpr (XF) {
        // K22f: the row's running power-of-two scale, the f16 hi | lo split and, where the scale fell, the accumulators' rescale
        lna_xf_scale_split<LNA_RG, T>(xc, kc, xs_cur, xinv, xh, xl, acc, w_scale, xs_cap, xs_cap_inv, a.row_add != nullptr);
      }
      // this chunk's weights (DMA issued one iteration ago, before that iteration's MFMAs) have landed; the raw barrier
      // carries no fence, so nothing else is drained with them
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();  // + every wave is done reading buffer buf^1
      asm volatile("" ::: "memory");
      if (kc + 1 < nkc) {
        stage_w(kc + 1, buf ^ 1);
        load_x(kc + 1, xc);
      }
      else if (blk + blk_step < nblk) {  // first chunk of the next row block
        stage_w(0, buf ^ 1);
        set_rows(blk + blk_step);
        load_x(0, xc);
        fetch_addend_index(blk + blk_step);
      }
      const uint4* wc = wbuf + buf * CHUNK_U4;
      // Two channel tiles x LNA_RG row groups = 4 independent accumulators per product term: consecutive MFMAs never hit
      // the same accumulator
      if constexpr (XM != 0) {
        lna_mfma_f16_chunk<LNA_RG, T>(wc, lane, xh, xl, acc);
      } else {
#pragma unroll
      for (int t = 0; t < T; t += 2) {
        lna_bf16x8 wfr[2][3];
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) {
          const uint4* wf = wc + ((t + tt) * 3) * 64 + lane;
#pragma unroll
          for (int pl = 0; pl < 3; ++pl) wfr[tt][pl] = __builtin_bit_cast(lna_bf16x8, wf[64 * pl]);
        }
        // (weight plane, x plane) of the six leading cross terms, small ones first
        constexpr int TERM_W[6] = {2, 0, 1, 1, 0, 0};
        constexpr int TERM_X[6] = {0, 2, 1, 0, 1, 0};
#pragma unroll
        for (int term = 0; term < 6; ++term)
#pragma unroll
          for (int tt = 0; tt < 2; ++tt)
#pragma unroll
            for (int rg = 0; rg < LNA_RG; ++rg) {
              const lna_u32x4 xb = TERM_X[term] == 0 ? xh[rg] : TERM_X[term] == 1 ? xm[rg] : xl[rg];
              acc[rg][t + tt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wfr[tt][TERM_W[term]], __builtin_bit_cast(lna_bf16x8, xb),
                                                                        acc[rg][t + tt], 0, 0, 0);
            }
      }
      }
    }
    if constexpr (XM != 0) {  // back to the unscaled product: both scales are powers of two (exact)
      const float w_inv = reinterpret_cast<const float*>(a.planes)[FMT_HDR_INV_SCALE];
#pragma unroll
      for (int rg = 0; rg < LNA_RG; ++rg) {
        const float sc = xinv[rg] * w_inv;
#pragma unroll
        for (int t = 0; t < T; ++t) acc[rg][t] = acc[rg][t] * sc;
      }
    }
    if constexpr (SEG) {  // (`buf` was flipped by the loop: the chunk loop's last buffer, free now, is buf ^ 1)
      float* slots = reinterpret_cast<float*>(wbuf + (buf ^ 1) * CHUNK_U4);
      sb.blk_row0 = blk * LNA_ROWS; sb.wave = wave; sb.slots = slots; sb.sm = segsm;
      __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): this wave's LDS reads of the last chunk have returned ...
      __builtin_amdgcn_s_barrier();        // ... and so have every other wave's: the slots may overlay that buffer
      if (lane < 4) segsm->slot_sid[4 * wave + lane] = -1;
      lna_epilogue<T, true, NORM_CT, ACT_CT>(a_epi, acc, row0, ch_base, rowl, grp, vec, &sb);
      lna_seg_merge(a, slots, segsm);
    } else {
      lna_epilogue<T, false>(a_epi, acc, row0, ch_base, rowl, grp, vec);
    }
  }
}

}  // namespace fsf

using namespace fsf;

// 16-channel tiles of the launched kernel variant (the prepared weight is laid out for exactly this count)
static int lna_tiles(int c) {
  const int t = (c + 15) / 16;
  return t <= 2 ? 2 : (t <= 4 ? 4 : 8);
}

static int lna_slices(int c) { return (c + 127) / 128; }

extern "C" int64_t fsf_linear_prepared_weight_bytes(int32_t k, int32_t c) {
  if (k < 1 || c < 1) return 0;
  const int64_t nkc = (k + LNA_KC - 1) / LNA_KC;
  return lna_slices(c) * nkc * lna_tiles(c) * 3 * 64 * 16;
}

extern "C" int fsf_linear_prepare_weight(const float* weight, int32_t k, int32_t c, void* planes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!weight || !planes || k < 1 || c < 1) return FSF_ERR_INVALID_ARG;
  const int T = lna_tiles(c), nkc = (k + LNA_KC - 1) / LNA_KC, nslice = lna_slices(c);
  const int64_t total = (int64_t)nslice * nkc * T * 64;
  hipLaunchKernelGGL(lna_prepare_kernel, dim3(fsf_stream_grid(total, 256)), dim3(256), 0, stream, weight, (int)k, (int)c, T, nkc,
                     nslice, 128, (uint4*)planes);
  FSF_LAUNCH_CHECK();
  return FSF_OK;
}

// "sliced": nslice independent layers of slice_c output channels each, side by side in one launch (weight rows
// [s * slice_c, (s + 1) * slice_c) belong to layer s)
extern "C" int64_t fsf_linear_prepared_weight_sliced_bytes(int32_t k, int32_t nslice, int32_t slice_c) {
  if (k < 1 || nslice < 1 || slice_c < 1 || slice_c > 128) return 0;
  const int64_t nkc = (k + LNA_KC - 1) / LNA_KC;
  return (int64_t)nslice * nkc * lna_tiles(slice_c) * 3 * 64 * 16;
}

extern "C" int fsf_linear_prepare_weight_sliced(const float* weight, int32_t k, int32_t nslice, int32_t slice_c, void* planes,
                                                void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!weight || !planes || k < 1 || nslice < 1 || slice_c < 1 || slice_c > 128) return FSF_ERR_INVALID_ARG;
  const int T = lna_tiles(slice_c), nkc = (k + LNA_KC - 1) / LNA_KC;
  const int64_t total = (int64_t)nslice * nkc * T * 64;
  hipLaunchKernelGGL(lna_prepare_kernel, dim3(fsf_stream_grid(total, 256)), dim3(256), 0, stream, weight, (int)k,
                     (int)(nslice * slice_c), T, nkc, (int)nslice, (int)slice_c, (uint4*)planes);
  FSF_LAUNCH_CHECK();
  return FSF_OK;
}

static int lna_launch(const LnaArgs& a_in, int nslice, hipStream_t stream, bool xp = false, bool xf = false) {
  LnaArgs a = a_in;
  const int T = lna_tiles(a.slice_w < a.c ? a.slice_w : a.c);
  const int64_t nblk = (a.n + LNA_ROWS - 1) / LNA_ROWS;
  int64_t gx = (256 * (a.seg_out ? LNA_SEG_WPS : LNA_WPS) + nslice - 1) / nslice;
  if (gx > nblk) gx = nblk;
  if (xp) {  // K22h: 1-D grid, `gx` row-block lanes (a multiple of 8: one XCD per lane) x nslice workgroups each
    if (T != 8 || a.seg_out) return FSF_ERR_UNSUPPORTED;
    gx = (gx + 7) / 8 * 8;
    constexpr size_t smem = (size_t)2 * 8 * 2 * 64 * 16 + 384 * 4;
    static std::atomic<uint64_t> attr_done{0};
    FSF_HIP_TRY(fsf_set_max_dynamic_lds((const void*)linear_norm_act_kernel<8, false, -1, -1, true>, (int)smem, attr_done));
    hipLaunchKernelGGL((linear_norm_act_kernel<8, false, -1, -1, true>), dim3((unsigned)(gx * nslice)), dim3(256), smem, stream, a);
    FSF_LAUNCH_CHECK();
    return FSF_OK;
  }
  const dim3 grid((unsigned)gx, (unsigned)nslice);
#define FSF_LNA_X(T_, SEG_, NORM_, ACT_, XM_)                                                                                       \
  do {                                                                                                                              \
    constexpr size_t smem = (size_t)2 * T_ * (XM_ ? 2 : 3) * 64 * 16 + 384 * 4 + (SEG_ ? sizeof(LnaSegSmem) : 0);                   \
    static std::atomic<uint64_t> attr_done{0};                                                                                      \
    FSF_HIP_TRY(fsf_set_max_dynamic_lds((const void*)linear_norm_act_kernel<T_, SEG_, NORM_, ACT_, XM_>, (int)smem, attr_done));    \
    hipLaunchKernelGGL((linear_norm_act_kernel<T_, SEG_, NORM_, ACT_, XM_>), grid, dim3(LNA_NW * 64), smem, stream, a);             \
  } while (0)
#define FSF_LNA(T_, SEG_, NORM_, ACT_) FSF_LNA_X(T_, SEG_, NORM_, ACT_, 0)
  if (xf) {  // K22f: the 64- and 128-channel-tile forms (what the SIR / VFE / segmentation-head layers are)
    if (a.seg_out) {
      if (a.norm != 1 || (a.act != 1 && a.act != 2)) return FSF_ERR_UNSUPPORTED;
      if (T == 4 && a.act == 2) FSF_LNA_X(4, true, 1, 2, 2);
      else if (T == 4) FSF_LNA_X(4, true, 1, 1, 2);
      else if (T == 8 && a.act == 2) FSF_LNA_X(8, true, 1, 2, 2);
      else if (T == 8) FSF_LNA_X(8, true, 1, 1, 2);
      else return FSF_ERR_UNSUPPORTED;
    } else if (T == 4) FSF_LNA_X(4, false, -1, -1, 2);
    else if (T == 8) FSF_LNA_X(8, false, -1, -1, 2);
    else return FSF_ERR_UNSUPPORTED;
    FSF_LAUNCH_CHECK();
    return FSF_OK;
  }
  if (a.seg_out) {  // K22s: LayerNorm + GELU / ReLU (the SIR layers), 36 .. 128 channels
    if (a.norm != 1 || (a.act != 1 && a.act != 2)) return FSF_ERR_UNSUPPORTED;
    if (T == 4 && a.act == 2) FSF_LNA(4, true, 1, 2);
    else if (T == 4) FSF_LNA(4, true, 1, 1);
    else if (T == 8 && a.act == 2) FSF_LNA(8, true, 1, 2);
    else if (T == 8) FSF_LNA(8, true, 1, 1);
    else return FSF_ERR_UNSUPPORTED;
  } else if (T == 2) FSF_LNA(2, false, -1, -1);
  else if (T == 4) FSF_LNA(4, false, -1, -1);
  else FSF_LNA(8, false, -1, -1);
#undef FSF_LNA
#undef FSF_LNA_X
  FSF_LAUNCH_CHECK();
  return FSF_OK;
}

extern "C" int fsf_linear_norm_act_sliced(const float* x, int64_t n, int32_t k, int64_t x_stride, int64_t x_slice_offset,
                                          const void* planes, int32_t nslice, int32_t slice_c, const float* bias, int32_t norm,
                                          const float* gamma, const float* beta, float eps, int32_t act, float* out,
                                          int64_t out_stride, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (n < 0 || k < 1 || nslice < 1 || slice_c < 1 || !planes || norm < 0 || norm > 2 || act < 0 || act > 2 ||
      (norm != 0 && (!gamma || !beta)) || (n > 0 && (!x || !out)) || x_slice_offset < 0)
    return FSF_ERR_INVALID_ARG;
  if (slice_c > 128 || (slice_c % 4) != 0 || (x_stride % 4) != 0 || (x_slice_offset % 4) != 0 || (out_stride % 4) != 0 ||
      ((uintptr_t)x % 16) != 0 || ((uintptr_t)out % 16) != 0)
    return FSF_ERR_UNSUPPORTED;
  if (x_stride < (int64_t)(nslice - 1) * x_slice_offset + k || out_stride < (int64_t)nslice * slice_c) return FSF_ERR_INVALID_ARG;
  if (n == 0) return FSF_OK;
  LnaArgs a{x, x_stride, (int)k, (const uint4*)planes, bias, gamma, beta, eps, (int)norm, (int)act, out, out_stride, n,
            (int)(nslice * slice_c), nullptr, nullptr, 0, (int)slice_c, (int)slice_c, x_slice_offset, nullptr, nullptr, 0, nullptr};
  return lna_launch(a, nslice, stream);
}

extern "C" int fsf_linear_norm_act_grouped(const float* x, int64_t n, int32_t k, int64_t x_stride, const void* planes, int32_t c,
                                           const float* bias, const float* row_add, const int64_t* row_add_index,
                                           int64_t row_add_stride, int32_t norm, const float* gamma, const float* beta,
                                           float eps, int32_t act, float* out, int64_t out_stride, void* stream_);

extern "C" int fsf_linear_norm_act(const float* x, int64_t n, int32_t k, int64_t x_stride, const void* planes, int32_t c,
                                   const float* bias, int32_t norm, const float* gamma, const float* beta, float eps,
                                   int32_t act, float* out, int64_t out_stride, void* stream_) {
  return fsf_linear_norm_act_grouped(x, n, k, x_stride, planes, c, bias, nullptr, nullptr, 0, norm, gamma, beta, eps, act, out,
                                     out_stride, stream_);
}

static int lna_grouped(const float* x, int64_t n, int32_t k, int64_t x_stride, const void* planes, int32_t c, const float* bias,
                       const float* row_add, const int64_t* row_add_index, int64_t row_add_stride, int32_t norm, const float* gamma,
                       const float* beta, float eps, int32_t act, float* out, int64_t out_stride, void* stream_, bool xf) {
  hipStream_t stream = (hipStream_t)stream_;
  if (n > 0 && (row_add == nullptr) != (row_add_index == nullptr)) return FSF_ERR_INVALID_ARG;  // (no rows: the index of no rows may be NULL)
  if (xf && (c <= 32 || ((uintptr_t)planes % 16) != 0)) return FSF_ERR_UNSUPPORTED;
  if (row_add && ((row_add_stride % 4) != 0 || row_add_stride < c || ((uintptr_t)row_add % 16) != 0)) return FSF_ERR_UNSUPPORTED;
  if (n < 0 || k < 1 || c < 1 || !planes || norm < 0 || norm > 2 || act < 0 || act > 2 || (norm != 0 && (!gamma || !beta)) ||
      (n > 0 && (!x || !out)))
    return FSF_ERR_INVALID_ARG;
  // 16-byte row accesses: x rows and out rows must be 16-byte aligned, c a multiple of 4
  if ((c > 128 && norm == 1) || (c % 4) != 0 || (x_stride % 4) != 0 || (out_stride % 4) != 0 || ((uintptr_t)x % 16) != 0 ||
      ((uintptr_t)out % 16) != 0)
    return FSF_ERR_UNSUPPORTED;
  if (x_stride < k || out_stride < c) return FSF_ERR_INVALID_ARG;
  if (n == 0) return FSF_OK;
  LnaArgs a{x, x_stride, (int)k, (const uint4*)planes, bias, gamma, beta, eps, (int)norm, (int)act, out, out_stride, n, (int)c,
            row_add, row_add_index, row_add_stride, 128, (int)c, 0, nullptr, nullptr, 0, nullptr};
  return lna_launch(a, lna_slices(c), stream, false, xf);
}

extern "C" int fsf_linear_norm_act_grouped(const float* x, int64_t n, int32_t k, int64_t x_stride, const void* planes, int32_t c,
                                           const float* bias, const float* row_add, const int64_t* row_add_index,
                                           int64_t row_add_stride, int32_t norm, const float* gamma, const float* beta,
                                           float eps, int32_t act, float* out, int64_t out_stride, void* stream_) {
  return lna_grouped(x, n, k, x_stride, planes, c, bias, row_add, row_add_index, row_add_stride, norm, gamma, beta, eps, act, out,
                     out_stride, stream_, false);
}

extern "C" int fsf_linear_f16w_norm_act_grouped(const float* x, int64_t n, int32_t k, int64_t x_stride, const void* w_planes, int32_t c,
                                                const float* bias, const float* row_add, const int64_t* row_add_index,
                                                int64_t row_add_stride, int32_t norm, const float* gamma, const float* beta,
                                                float eps, int32_t act, float* out, int64_t out_stride, void* stream_) {
  return lna_grouped(x, n, k, x_stride, w_planes, c, bias, row_add, row_add_index, row_add_stride, norm, gamma, beta, eps, act, out,
                     out_stride, stream_, true);
}

static int lna_segmax(const float* x, int64_t n, int32_t k, int64_t x_stride, const void* planes, int32_t c, const float* bias,
                      const float* row_add, const int64_t* row_add_index, int64_t row_add_stride, int32_t norm, const float* gamma,
                      const float* beta, float eps, int32_t act, const int64_t* seg_ids, int64_t num_segments, float* seg_out,
                      int64_t seg_out_stride, float* out, int64_t out_stride, void* stream_, bool xf) {
  hipStream_t stream = (hipStream_t)stream_;
  if (xf && planes && ((uintptr_t)planes % 16) != 0) return FSF_ERR_UNSUPPORTED;
  if (n > 0 && (row_add == nullptr) != (row_add_index == nullptr)) return FSF_ERR_INVALID_ARG;  // (no rows: the index of no rows may be NULL)
  if (row_add && ((row_add_stride % 4) != 0 || row_add_stride < c || ((uintptr_t)row_add % 16) != 0)) return FSF_ERR_UNSUPPORTED;
  if (n < 0 || k < 1 || c < 1 || !planes || norm < 0 || norm > 2 || act < 0 || act > 2 || (norm != 0 && (!gamma || !beta)) ||
      num_segments < 0 || (n > 0 && (!x || !seg_ids || !seg_out || num_segments < 1)))
    return FSF_ERR_INVALID_ARG;
  // LayerNorm + ReLU / GELU (what SIRLayer puts in front of its max), one 128-channel slice at most, more than 32 channels (the
  // slots overlay a >= 12 KB weight buffer)
  if (norm != 1 || act == 0 || c > 128 || c <= 32 || (c % 4) != 0 || (x_stride % 4) != 0 || ((uintptr_t)x % 16) != 0 || (seg_out_stride % 4) != 0 ||
      seg_out_stride < c || ((uintptr_t)seg_out % 16) != 0 || (out && ((out_stride % 4) != 0 || ((uintptr_t)out % 16) != 0)) ||
      n >= ((int64_t)1 << 31) || num_segments >= LNA_SLOT_HEAD_OPEN || num_segments * seg_out_stride >= ((int64_t)1 << 31))
    return FSF_ERR_UNSUPPORTED;
  if (x_stride < k || (out && out_stride < c)) return FSF_ERR_INVALID_ARG;
  if (n == 0) return FSF_OK;
  LnaArgs a{x, x_stride, (int)k, (const uint4*)planes, bias, gamma, beta, eps, (int)norm, (int)act, out, out_stride, n, (int)c,
            row_add, row_add_index, row_add_stride, 128, (int)c, 0, seg_ids, seg_out, seg_out_stride, nullptr};
  return lna_launch(a, 1, stream, false, xf);
}

extern "C" int fsf_linear_norm_act_segmax(const float* x, int64_t n, int32_t k, int64_t x_stride, const void* planes, int32_t c,
                                          const float* bias, const float* row_add, const int64_t* row_add_index,
                                          int64_t row_add_stride, int32_t norm, const float* gamma, const float* beta, float eps,
                                          int32_t act, const int64_t* seg_ids, int64_t num_segments,
                                          float* seg_out, int64_t seg_out_stride, float* out, int64_t out_stride, void* stream_) {
  return lna_segmax(x, n, k, x_stride, planes, c, bias, row_add, row_add_index, row_add_stride, norm, gamma, beta, eps, act, seg_ids,
                    num_segments, seg_out, seg_out_stride, out, out_stride, stream_, false);
}

extern "C" int fsf_linear_f16w_norm_act_segmax(const float* x, int64_t n, int32_t k, int64_t x_stride, const void* w_planes, int32_t c,
                                               const float* bias, const float* row_add, const int64_t* row_add_index,
                                               int64_t row_add_stride, int32_t norm, const float* gamma, const float* beta, float eps,
                                               int32_t act, const int64_t* seg_ids, int64_t num_segments,
                                               float* seg_out, int64_t seg_out_stride, float* out, int64_t out_stride, void* stream_) {
  return lna_segmax(x, n, k, x_stride, w_planes, c, bias, row_add, row_add_index, row_add_stride, norm, gamma, beta, eps, act, seg_ids,
                    num_segments, seg_out, seg_out_stride, out, out_stride, stream_, true);
}

// ---- K22h entry points ---------------------------------------------------------------------------------------------------
extern "C" int64_t fsf_linear_prepared_weight_f16_bytes(int32_t k, int32_t c, int32_t slice_c) {
  if (k < 1 || c < 1 || slice_c < 1 || slice_c > 128) return 0;
  const int64_t nkc = (k + LNA_KC - 1) / LNA_KC, nslice = (c + slice_c - 1) / slice_c;
  return FMT_HDR_BYTES + nslice * nkc * lna_tiles(slice_c) * 2 * 64 * 16;
}

extern "C" int fsf_linear_prepare_weight_f16(const float* weight, int32_t k, int32_t c, int32_t slice_c, void* planes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!weight || !planes || k < 1 || c < 1 || slice_c < 1 || slice_c > 128) return FSF_ERR_INVALID_ARG;
  if (((uintptr_t)planes % 16) != 0) return FSF_ERR_UNSUPPORTED;
  const int T = lna_tiles(slice_c), nkc = (k + LNA_KC - 1) / LNA_KC, nslice = (c + slice_c - 1) / slice_c;
  const int rc = fsf_weight_layer_absmax(weight, (int64_t)c * k, planes, stream);
  if (rc != FSF_OK) return rc;
  const int64_t total = (int64_t)nslice * nkc * T * 64;
  hipLaunchKernelGGL(lna_prepare_f16_kernel, dim3(fsf_stream_grid(total, 256)), dim3(256), 0, stream, weight, (int)k, (int)c, T, nkc,
                     nslice, (int)slice_c, (float*)planes, (uint4*)planes + FMT_HDR_U4);
  FSF_LAUNCH_CHECK();
  return FSF_OK;
}

extern "C" int64_t fsf_row_planes_bytes(int64_t n, int32_t c) { return (n < 0 || c < 8 || (c % 8) != 0) ? 0 : n * (int64_t)c * 4; }

extern "C" int fsf_rows_to_planes(const float* x, int64_t n, int32_t c, int64_t x_stride, int32_t norm, const float* gamma,
                                  const float* beta, float eps, int32_t act, void* planes, float* inv_scales, float* out,
                                  int64_t out_stride, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (n < 0 || c < 8 || norm < 0 || norm > 1 || act < 0 || act > 2 || (norm == 1 && (!gamma || !beta)) ||
      (n > 0 && (!x || !planes || !inv_scales)))
    return FSF_ERR_INVALID_ARG;
  if ((c % 8) != 0 || c > 2048 || (x_stride % 4) != 0 || x_stride < c || ((uintptr_t)x % 16) != 0 || ((uintptr_t)planes % 16) != 0 ||
      (out && ((out_stride % 4) != 0 || out_stride < c || ((uintptr_t)out % 16) != 0)) ||
      (norm == 1 && (((uintptr_t)gamma % 16) != 0 || ((uintptr_t)beta % 16) != 0)))
    return FSF_ERR_UNSUPPORTED;
  if (n == 0) return FSF_OK;
  const int bl = (c / 8 + 63) / 64;  // 8-channel blocks per lane
  int64_t g = (n + 3) / 4;
  if (g > 16384) g = 16384;
#define FSF_R2P(BL_, N_, A_)                                                                                                     \
  hipLaunchKernelGGL((rows_to_planes_kernel<BL_, N_, A_>), dim3((unsigned)g), dim3(256), 0, stream, x, n, (int)c, x_stride, gamma, \
                     beta, eps, (uint4*)planes, inv_scales, out, out_stride)
#define FSF_R2P_ACT(BL_, N_)                      \
  do {                                            \
    if (act == 0) FSF_R2P(BL_, N_, 0);            \
    else if (act == 1) FSF_R2P(BL_, N_, 1);       \
    else FSF_R2P(BL_, N_, 2);                     \
  } while (0)
  if (bl <= 1) { if (norm) FSF_R2P_ACT(1, 1); else FSF_R2P_ACT(1, 0); }
  else if (bl <= 2) { if (norm) FSF_R2P_ACT(2, 1); else FSF_R2P_ACT(2, 0); }
  else { if (norm) FSF_R2P_ACT(4, 1); else FSF_R2P_ACT(4, 0); }
#undef FSF_R2P_ACT
#undef FSF_R2P
  FSF_LAUNCH_CHECK();
  return FSF_OK;
}

extern "C" int fsf_linear_planes_norm_act(const void* x_planes, const float* x_inv_scales, int64_t n, int32_t k, const void* w_planes,
                                          int32_t c, int32_t slice_c, const float* bias, int32_t norm, const float* gamma,
                                          const float* beta, float eps, int32_t act, float* out, int64_t out_stride, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (n < 0 || k < 1 || c < 1 || slice_c < 1 || !w_planes || norm < 0 || norm > 2 || act < 0 || act > 2 ||
      (norm != 0 && (!gamma || !beta)) || (n > 0 && (!x_planes || !x_inv_scales || !out)))
    return FSF_ERR_INVALID_ARG;
  // whole 32-k chunks; 128-channel tiles (slice_c in 68..128 so that the launched variant is the 8-tile one); a LayerNorm spans ONE slice
  if ((k % 32) != 0 || slice_c > 128 || slice_c <= 64 || (slice_c % 4) != 0 || (c % 4) != 0 || (out_stride % 4) != 0 ||
      ((uintptr_t)x_planes % 16) != 0 || ((uintptr_t)w_planes % 16) != 0 || ((uintptr_t)out % 16) != 0)
    return FSF_ERR_UNSUPPORTED;
  if (out_stride < c) return FSF_ERR_INVALID_ARG;
  if (n == 0) return FSF_OK;
  const int nslice = (c + slice_c - 1) / slice_c;
  LnaArgs a{(const float*)x_planes, (int64_t)k, (int)k, (const uint4*)w_planes, bias, gamma, beta, eps, (int)norm, (int)act, out, out_stride, n,
            (int)c, nullptr, nullptr, 0, (int)slice_c, (int)slice_c, 0, nullptr, nullptr, 0, x_inv_scales};
  return lna_launch(a, nslice, stream, true);
}
