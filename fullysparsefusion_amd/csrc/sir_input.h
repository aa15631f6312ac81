// K21: what its kernel (csrc/sir_input.hip) shares with the fused K21 + first K22s layer (csrc/sir_linear.hip): the argument block and
// one wave's pass over a 16-row group — sources, position MLP, product — with the place the product goes left to the caller.
#pragma once
#include "common.h"

namespace fsf {

constexpr int SI_MAX_R = 16;   // f_cluster columns
constexpr int SI_MAX_H1 = 16;
constexpr int SI_MAX_H2 = 32;

struct SirInputArgs {
  const float* points; int64_t points_stride; int p_cols;
  const float* feats;  int64_t feats_stride;  int f_cols;   // f_cols = all feature columns (the sum over the parts below)
  // the feature columns may come from up to three tensors side by side (parts 1, 2 follow part 0), and their rows may be taken
  // through an index (row i of the layer input = row feats_index[i] of every part): the gather of the group-sampled points and
  // the [n, 11 + 33 + 131] concat the reference materialises before its first SIR layer happen in this kernel's loads
  const float* feats1; int64_t feats1_stride; int f0_cols, f1_cols;
  const float* feats2; int64_t feats2_stride;
  const int64_t* feats_index;
  int direct_mask;  // bit p: part p is NOT read through feats_index (its rows are already the layer's rows)
  const float* extra;  int64_t extra_stride;  int e_cols; float extra_div;
  const float* fcl;    int64_t fcl_stride;    int r_cols; float rel_div;
  float norm[3];
  const float *w1, *g1, *b1; int h1;
  const float *w2, *g2, *b2; int h2;
  const float *w3, *g3, *b3;
  float eps; int act;
  float* out; int64_t out_stride;
  int64_t n; int c;
};

// GELU: the library's one form (common.h: max(y, 0) - t 2^P(t), branch-free, one transcendental per value); the kernel is
// instruction-bound and libm's two-branch erff is 35 VALU ops + divergence per element, 60 elements per lane per 16 rows.
__device__ __forceinline__ float si_gelu(float y) { return fsf_gelu(y); }

__device__ __forceinline__ float si_act(float y, int act) {
  if (act == 1) return fmaxf(y, 0.0f);
  if (act == 2) return si_gelu(y);
  return y;
}

typedef float si_f32x4 __attribute__((ext_vector_type(4)));
typedef float si_f32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ si_f32x2 si_pk(float v) { return si_f32x2{v, v}; }
__device__ __forceinline__ si_f32x2 si_pk_fma(si_f32x2 a, si_f32x2 b, si_f32x2 c) { return __builtin_elementwise_fma(a, b, c); }

// The same GELU on TWO values per lane (v_pk_fma_f32 / v_pk_mul_f32 / v_pk_add_f32 issue at the rate of their scalar forms).
__device__ __forceinline__ si_f32x2 si_gelu2(si_f32x2 y) { return fsf_gelu2(y); }

__device__ __forceinline__ si_f32x2 si_act2(si_f32x2 y, int act) {
  if (act == 1) return si_f32x2{fmaxf(y.x, 0.0f), fmaxf(y.y, 0.0f)};
  if (act == 2) return si_gelu2(y);
  return y;
}

// sum over the 4 lanes that share a point row (lane = row + 16 * group)
__device__ __forceinline__ float si_row_sum(float v) {
  v += __shfl_xor(v, 16);
  v += __shfl_xor(v, 32);
  return v;
}

// The position MLP on the matrix cores, TRANSPOSED: out^T[channel, row] = W[channel, unit] x h^T[unit, row] with
// v_mfma_f32_16x16x4_f32, the weights as the A operand and 16 point rows as the B operand.  Lane (row = lane & 15,
// group = lane >> 4) then holds channels 16 t + 4 group + r (r = 0..3) of its row for every 16-channel tile t — which
// is exactly the B operand of the NEXT layer if that layer walks its units in the order (t, r): the three layers chain
// through registers with no cross-lane traffic, LayerNorm is an in-lane sum + two shuffles over the 4 lanes of a row,
// and the activation runs on 1/4 row per lane.  (Before: lane = row for the two thin layers and lane = channel for the
// wide one, all on the VALU — 9 k FMAs per row were ~40 % of its ~350 wave instructions per row.)
// The activated [16, C] tile goes through a per-wave LDS slice so that the product with the concatenated sources and
// the store run with lane = channel (coalesced rows).
// The body of K21 for one wave of a workgroup of NWAVES, with the walk over the 16-row groups and the place the products go left to
// `d` (the kernel of csrc/sir_input.hip stores them; the fused kernel of csrc/sir_linear.hip keeps them in the tile and multiplies on):
//   d.first() / d.next()   the first group of this wave, and the one after the current group (-1: none); next() is asked once per group,
//                          at its start, so that the next group's MLP input is requested one group ahead
//   d.begin(row0), then per row i (all 16 when Driver::ALL_ROWS, else the rows below n; rows past n repeat row n - 1 in every respect)
//   d.put(i, t, p, v) for the column lane + 64 t (p = its place in the wave's tile, v = x * h) and d.next_row();  d.end_group(tile)
// `si_smem`: si_smem_bytes<NT3, NWAVES>() of LDS, 16-byte aligned.  Contains one __syncthreads, before the first group.
template <int NT3, int NWAVES>
constexpr size_t si_smem_bytes() { return (size_t)(NT3 * 2 * 64 * 4 + 2 * NT3 * 16 + NWAVES * 16 * (NT3 * 16 + 4)) * sizeof(float); }

template <int NT3, int ACT, int NWAVES, class Driver>
__device__ __forceinline__ void si_run(const SirInputArgs& a, char* si_smem, Driver& d) {
  constexpr int TS = NT3 * 16 + 4;  // tile row stride (floats): 16-byte rows, 4-bank skew between rows
  float* w3f = reinterpret_cast<float*>(si_smem);  // [NT3][2][64 lanes][4]: layer-3 weights in fragment order
  float* g3s = w3f + NT3 * 2 * 64 * 4;             // [NT3 * 16]
  float* b3s = g3s + NT3 * 16;
  float* tiles = b3s + NT3 * 16;                   // [NWAVES][16 rows][TS]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int rowl = lane & 15, grp = lane >> 4;

  for (int idx = threadIdx.x; idx < NT3 * 2 * 64; idx += NWAVES * 64) {
    const int t3 = idx >> 7, t2 = (idx >> 6) & 1, l = idx & 63;
    const int out = 16 * t3 + (l & 15), in0 = 16 * t2 + 4 * (l >> 4);
#pragma unroll
    for (int r = 0; r < 4; ++r)
      w3f[idx * 4 + r] = (out < a.c && in0 + r < a.h2) ? a.w3[(int64_t)out * a.h2 + in0 + r] : 0.0f;
  }
  for (int t = threadIdx.x; t < NT3 * 16; t += NWAVES * 64) {
    g3s[t] = t < a.c ? a.g3[t] : 0.0f;
    b3s[t] = t < a.c ? a.b3[t] : 0.0f;
  }
  // layers 1 and 2: weight fragments and LayerNorm affine of this lane's channels, in registers for the whole kernel
  float w1f[4], g1r[4], b1r[4], w2f[2][4], g2r[2][4], b2r[2][4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int in = 4 * grp + r;  // A operand: lane (m = rowl, group) supplies W[m][4 group + r]
    w1f[r] = (rowl < a.h1 && in < a.r_cols) ? a.w1[rowl * a.r_cols + in] : 0.0f;
    g1r[r] = in < a.h1 ? a.g1[in] : 0.0f;  // D: the same lane holds channel 4 group + r
    b1r[r] = in < a.h1 ? a.b1[in] : 0.0f;
#pragma unroll
    for (int t2 = 0; t2 < 2; ++t2) {
      w2f[t2][r] = (16 * t2 + rowl < a.h2 && in < a.h1) ? a.w2[(16 * t2 + rowl) * a.h1 + in] : 0.0f;
      g2r[t2][r] = 16 * t2 + in < a.h2 ? a.g2[16 * t2 + in] : 0.0f;
      b2r[t2][r] = 16 * t2 + in < a.h2 ? a.b2[16 * t2 + in] : 0.0f;
    }
  }
  __syncthreads();

  // lane = channel view of the concatenated sources: column lane + 64 t lives in ONE of the three tensors
  constexpr int T = (NT3 * 16 + 63) / 64;
  const float* xsrc[T];
  int64_t xstride[T];
  float xdiv[T];
  bool xgath[T];  // this lane's column of tile t is read through feats_index
#pragma unroll
  for (int t = 0; t < T; ++t) {
    const int c = lane + 64 * t;
    xgath[t] = false;
    xsrc[t] = a.points;  // (columns >= c read a valid address and are never stored)
    xstride[t] = a.points_stride;
    xdiv[t] = 1.0f;
    if (c < a.p_cols) {
      xsrc[t] = a.points + c;
      if (c < 3) xdiv[t] = a.norm[c];
    } else if (c < a.p_cols + a.f_cols) {
      const int fc = c - a.p_cols;
      int part = 0;
      if (fc < a.f0_cols) {
        xsrc[t] = a.feats + fc;
        xstride[t] = a.feats_stride;
      } else if (fc < a.f0_cols + a.f1_cols) {
        xsrc[t] = a.feats1 + (fc - a.f0_cols);
        xstride[t] = a.feats1_stride;
        part = 1;
      } else {
        xsrc[t] = a.feats2 + (fc - a.f0_cols - a.f1_cols);
        xstride[t] = a.feats2_stride;
        part = 2;
      }
      xgath[t] = a.feats_index != nullptr && !((a.direct_mask >> part) & 1);
    } else if (c < a.c) {
      xsrc[t] = a.extra + (c - a.p_cols - a.f_cols);
      xstride[t] = a.extra_stride;
      xdiv[t] = a.extra_div;
    }
  }
  bool xneed[T];  // wave-uniform: does 64-column tile t hold a column that is divided (xyz, or `extra`)?
#pragma unroll
  for (int t = 0; t < T; ++t) xneed[t] = t == 0 || (a.e_cols > 0 && 64 * t + 63 >= a.p_cols + a.f_cols && 64 * t < a.c);
  float* tile = tiles + wave * 16 * TS;
  const float inv_h1 = 1.0f / (float)a.h1, inv_h2 = 1.0f / (float)a.h2, inv_c = 1.0f / (float)a.c;
  // MFMA-layout load of the layer-1 input (f_cluster) of a group: lane (row, group) reads columns 4 group + r
  auto load_fcl = [&](int64_t gi, float (&v)[4]) {
    const int64_t r0 = gi * 16;
    const int nr = (int)min((int64_t)16, a.n - r0);
    const int64_t rc = r0 + (rowl < nr ? rowl : nr - 1);  // rows past n repeat the last one (finite, never stored)
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = 4 * grp + r < a.r_cols ? a.fcl[rc * a.fcl_stride + 4 * grp + r] : 0.0f;
  };
  // the group's feature-row indices, lane (row, .) holds its row's: requested one group ahead like the MLP input
  auto load_idx = [&](int64_t gi) -> int {
    if (!a.feats_index) return 0;
    const int64_t r0 = gi * 16;
    const int nr = (int)min((int64_t)16, a.n - r0);
    return (int)a.feats_index[r0 + (rowl < nr ? rowl : nr - 1)];
  };
  float xnext[4] = {0.f, 0.f, 0.f, 0.f};
  int inext = 0;
  int64_t gi = d.first();
  if (gi >= 0) {
    load_fcl(gi, xnext);
    inext = load_idx(gi);
  }
  while (gi >= 0) {
    const int64_t gi_next = d.next();
    const int64_t row0 = gi * 16;
    const int nrow = (int)min((int64_t)16, a.n - row0);
    // ---- the group's sources are requested first, lane = channel: 16 rows x T loads per lane stay in flight under the
    // whole position MLP (a wave has only one other wave on its SIMD to hide HBM latency behind)
    // (the MLP input of the NEXT group is requested here too: it is the first thing a group needs, and waiting for it
    // with nothing else to do was 40 % of the wave cycles)
    float xin[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) xin[r] = xnext[r];
    const int icur = inext;
    if (gi_next >= 0) {
      load_fcl(gi_next, xnext);
      inext = load_idx(gi_next);
    }
    float x[16][T];
    if (a.feats_index) {  // (wave-uniform) gathered feature rows: row i of the group reads row readlane(icur, i) of the feature parts
      // Address of (row i, tile t) = cur[t] + ri * gstr[t]: the lane's columns that are NOT gathered walk down the group by their
      // stride (cur[t], one 64-bit add per load), the gathered ones add the row index — a scalar — times their stride in ONE
      // v_mad_u64_u32 (32 x 32 + 64 bits: indices and strides fit 32 bits, checked at launch).  As `(gathered ? ri : rr) * stride` in
      // 64 bits every load cost two selects and a 64 x 64-bit multiply: ~190 quarter-rate integer ops per 16-row group.
      const float* cur[T];
      uint32_t gstr[T];
      int64_t step[T];
#pragma unroll
      for (int t = 0; t < T; ++t) {
        cur[t] = xgath[t] ? xsrc[t] : xsrc[t] + row0 * xstride[t];
        gstr[t] = xgath[t] ? (uint32_t)xstride[t] : 0u;
        step[t] = xgath[t] ? 0 : xstride[t];
      }
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const uint32_t ri = (uint32_t)__builtin_amdgcn_readlane(icur, i);   // (rows past n repeat the last one: see load_idx)
#pragma unroll
        for (int t = 0; t < T; ++t) {
          x[i][t] = *(cur[t] + (uint64_t)ri * (uint64_t)gstr[t]);
          if (i + 1 < nrow) cur[t] += step[t];  // (wave-uniform)
        }
      }
    } else {
      const float* rp[T];  // row pointers walk down the group: one 64-bit add per load instead of a 64-bit multiply
#pragma unroll
      for (int t = 0; t < T; ++t) rp[t] = xsrc[t] + row0 * xstride[t];
#pragma unroll
      for (int i = 0; i < 16; ++i) {
#pragma unroll
        for (int t = 0; t < T; ++t) {
          x[i][t] = *rp[t];
          if (i + 1 < nrow) rp[t] += xstride[t];  // (wave-uniform; rows past n repeat the last one)
        }
      }
    }
    // ---- layer 1: K = r_cols (<= 16), one MFMA per r
    si_f32x4 acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < 4; ++r) xin[r] = 4 * grp + r < a.r_cols ? __fdiv_rn(xin[r], a.rel_div) : 0.0f;
#pragma unroll
    for (int r = 0; r < 4; ++r) acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(w1f[r], xin[r], acc1, 0, 0, 0);
    float h1v[4];
    {
      float s = 0.0f;
#pragma unroll
      for (int r = 0; r < 4; ++r) s += 4 * grp + r < a.h1 ? acc1[r] : 0.0f;
      const float mean = si_row_sum(s) * inv_h1;
      float q = 0.0f;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float d = 4 * grp + r < a.h1 ? acc1[r] - mean : 0.0f;
        q += d * d;
      }
      const float rstd = rsqrtf(si_row_sum(q) * inv_h1 + a.eps);
#pragma unroll
      for (int r = 0; r < 4; r += 2) {
        const si_f32x2 y = si_act2((si_f32x2{acc1[r], acc1[r + 1]} - si_pk(mean)) * si_pk(rstd) * si_f32x2{g1r[r], g1r[r + 1]} +
                                   si_f32x2{b1r[r], b1r[r + 1]}, ACT);
        h1v[r] = 4 * grp + r < a.h1 ? y.x : 0.0f;
        h1v[r + 1] = 4 * grp + r + 1 < a.h1 ? y.y : 0.0f;
      }
    }
    // ---- layer 2: two 16-channel tiles, K = h1
    si_f32x4 acc2[2];
#pragma unroll
    for (int t2 = 0; t2 < 2; ++t2) {
      acc2[t2] = si_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int r = 0; r < 4; ++r) acc2[t2] = __builtin_amdgcn_mfma_f32_16x16x4f32(w2f[t2][r], h1v[r], acc2[t2], 0, 0, 0);
    }
    float h2v[2][4];
    {
      float s = 0.0f;
#pragma unroll
      for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
        for (int r = 0; r < 4; ++r) s += 16 * t2 + 4 * grp + r < a.h2 ? acc2[t2][r] : 0.0f;
      const float mean = si_row_sum(s) * inv_h2;
      float q = 0.0f;
#pragma unroll
      for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float d = 16 * t2 + 4 * grp + r < a.h2 ? acc2[t2][r] - mean : 0.0f;
          q += d * d;
        }
      const float rstd = rsqrtf(si_row_sum(q) * inv_h2 + a.eps);
#pragma unroll
      for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
        for (int r = 0; r < 4; r += 2) {
          const si_f32x2 y = si_act2((si_f32x2{acc2[t2][r], acc2[t2][r + 1]} - si_pk(mean)) * si_pk(rstd) *
                                     si_f32x2{g2r[t2][r], g2r[t2][r + 1]} + si_f32x2{b2r[t2][r], b2r[t2][r + 1]}, ACT);
          h2v[t2][r] = 16 * t2 + 4 * grp + r < a.h2 ? y.x : 0.0f;
          h2v[t2][r + 1] = 16 * t2 + 4 * grp + r + 1 < a.h2 ? y.y : 0.0f;
        }
    }
    // ---- layer 3: NT3 tiles, K = h2 walked in (t2, r) order = the order the lanes hold h2v
    si_f32x4 acc3[NT3];
#pragma unroll
    for (int t3 = 0; t3 < NT3; ++t3) {
      acc3[t3] = si_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int t2 = 0; t2 < 2; ++t2) {
        const si_f32x4 wf = *reinterpret_cast<const si_f32x4*>(w3f + ((t3 * 2 + t2) * 64 + lane) * 4);
#pragma unroll
        for (int r = 0; r < 4; ++r) acc3[t3] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[r], h2v[t2][r], acc3[t3], 0, 0, 0);
      }
    }
    {
      // channels >= c have zero weights: their accumulators are exactly 0 and drop out of the sum; for the squared
      // deviations they are masked by a per-lane limit (kept opaque so the 4 NT3 compares are redone per group instead
      // of living in 2 x 4 NT3 scalar registers for the whole kernel)
      int lim = a.c - 4 * grp;
      asm volatile("" : "+v"(lim));
      si_f32x2 s2 = si_pk(0.0f);
#pragma unroll
      for (int t3 = 0; t3 < NT3; ++t3) s2 = (s2 + si_f32x2{acc3[t3][0], acc3[t3][1]}) + si_f32x2{acc3[t3][2], acc3[t3][3]};
      const float mean = si_row_sum(s2.x + s2.y) * inv_c;
      si_f32x2 q2 = si_pk(0.0f);
#pragma unroll
      for (int t3 = 0; t3 < NT3; ++t3)
#pragma unroll
        for (int r = 0; r < 4; r += 2) {
          si_f32x2 d = si_f32x2{acc3[t3][r], acc3[t3][r + 1]} - si_pk(mean);
          d.x = 16 * t3 + r < lim ? d.x : 0.0f;
          d.y = 16 * t3 + r + 1 < lim ? d.y : 0.0f;
          q2 = si_pk_fma(d, d, q2);
        }
      const float rstd = rsqrtf(si_row_sum(q2.x + q2.y) * inv_c + a.eps);
#pragma unroll
      for (int t3 = 0; t3 < NT3; ++t3) {
        const int ch0 = 16 * t3 + 4 * grp;
        const float4 gv = *reinterpret_cast<const float4*>(g3s + ch0), bv = *reinterpret_cast<const float4*>(b3s + ch0);
        const si_f32x2 yl = si_act2((si_f32x2{acc3[t3][0], acc3[t3][1]} - si_pk(mean)) * si_pk(rstd) * si_f32x2{gv.x, gv.y} +
                                    si_f32x2{bv.x, bv.y}, ACT);
        const si_f32x2 yh = si_act2((si_f32x2{acc3[t3][2], acc3[t3][3]} - si_pk(mean)) * si_pk(rstd) * si_f32x2{gv.z, gv.w} +
                                    si_f32x2{bv.z, bv.w}, ACT);
        *reinterpret_cast<float4*>(tile + rowl * TS + ch0) = make_float4(yl.x, yl.y, yh.x, yh.y);  // (channels >= c: affine 0 -> act(0) = 0, never read)
      }
    }
    // ---- product with the concatenated sources, lane = channel (the tile is private to this wave: its LDS writes are
    // ordered before these reads)
    d.begin(row0);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      if (Driver::ALL_ROWS || i < nrow) {  // wave-uniform
#pragma unroll
        for (int t = 0; t < T; ++t) {
          // true divisions, as the reference's `/` (x / 1 is exact), only in the tiles that hold a divided column: a REAL branch
          // (the empty volatile statement keeps the compiler from turning the wave-uniform test into a select, which ran the
          // thirteen-instruction IEEE division for every tile of every row: 48 per 16-row group at c = 180 where 16 are needed)
          float xv = x[i][t];
          if (xneed[t]) {
            asm volatile("" ::: "memory");
            xv = __fdiv_rn(xv, xdiv[t]);
          }
          d.put(i, t, tile + i * TS + lane + 64 * t, xv * tile[i * TS + lane + 64 * t]);
        }
        d.next_row();
      }
    }
    d.end_group(tile);
    gi = gi_next;
  }
}

}  // namespace fsf
