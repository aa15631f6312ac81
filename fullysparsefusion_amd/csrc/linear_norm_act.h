// K22 family: the device functions its kernels share (csrc/linear_norm_act.hip: K22 / K22s / K22f / K22h; csrc/sir_linear.hip: the
// fused K21 + first K22s layer).  See include/fsf_hip.h and docs/kernels/K21_K22_linear_family.md.
#pragma once
#include "common.h"
#include "operand_formats.h"

namespace fsf {

typedef __bf16 lna_bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 lna_f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 lna_f16x4 __attribute__((ext_vector_type(4)));
typedef float lna_f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned lna_u32x4 __attribute__((ext_vector_type(4)));

constexpr int LNA_KC = 32;        // k per LDS chunk (one MFMA k step)
constexpr int LNA_NW = 4;         // waves per workgroup (two workgroups per CU: one wave of each per SIMD)
constexpr int LNA_RG = 2;         // 16-row groups per wave and iteration
#ifndef LNA_WPS
#define LNA_WPS 3                 // waves per SIMD the register budget is set for (workgroups per CU)
#endif
#ifndef LNA_SEG_WPS
#define LNA_SEG_WPS 3             // ... of the K22s variants (2 = no spills at 256 registers, a third fewer waves: measured, see DESIGN)
#endif
constexpr int LNA_ROWS = LNA_NW * LNA_RG * 16;  // rows per workgroup iteration (4-wave workgroups)

struct LnaArgs {
  const float* x; int64_t x_stride; int k;
  const uint4* planes;  // [slice][KP/32][T][3][64 lanes] x 16 B (slice = 128 output channels)
  const float *bias, *gamma, *beta;
  float eps; int norm, act;  // norm 0 none / 1 LayerNorm / 2 affine (y * gamma + beta); act 0 / 1 ReLU / 2 GELU(erf)
  float* out; int64_t out_stride;
  int64_t n; int c;
  // optional per-row addend before the norm: row_add[row_add_index[row]][c] — the right half of a
  // `cat([point_feats, group_feats[inv]], 1) @ W^T` product, applied to the groups once instead of to every point
  const float* row_add; const int64_t* row_add_index; int64_t row_add_stride;
  // output channels per blockIdx.y slice (128 unless "sliced": independent layers side by side, one per slice), the width a
  // LayerNorm spans (c, or the slice width), and the column offset between the inputs of consecutive slices
  int slice_w, norm_w; int64_t x_slice_off;
  // fused segmented max (K22s): rows arrive SORTED by segment (seg_ids nondecreasing); seg_out[s, ch] = max over the rows of
  // segment s of the activated output.  seg_out must hold -inf on entry (a segment that reaches beyond one 128-row block is
  // combined with atomic max).  `out` may then be null.
  const int64_t* seg_ids; float* seg_out; int64_t seg_out_stride;
  // K22h (XP): `x` is the input in PLANE form — [row][k / 8][2][8] f16 hi | lo of x * s_row (rows_to_planes_kernel below; the layout
  // of fsf_to_planes with ONE power-of-two scale per row) —, x_inv_scale[row] = 1 / s_row, `planes` = f16 hi | lo fragments of
  // W * s_w behind a 256-byte header whose first float is 1 / s_w.  The product runs as three v_mfma_f32_16x16x32_f16 per
  // fp32-equivalent one (hi hi + hi lo + lo hi, as K9d), no split in the main loop.
  // The scale rules of the f16 forms (what tests/product_budget.py derives the per-element floors from): x — K22h: one s_row per row over
  // all k columns; K22f: per row, following the running maximum over the LNA_KC-column chunks (lna_xf_scale_split); W — K22f and K22h:
  // ONE power-of-two scale s_w for the whole layer (s_w * max |w| in [2^13, 2^14), lna_prepare_f16_kernel), whatever the slice width.
  const float* x_inv_scale;
};

// max of two floats into memory, any signs, by integer atomics on the IEEE bit patterns (target initialised to -inf): a value
// >= 0 orders like a signed int above every negative pattern, a value < 0 orders inversely as an unsigned int below every
// non-negative pattern's... (min over unsigned: non-negative patterns are the smallest, so a stored non-negative survives).
__device__ __forceinline__ void lna_atomic_max(float* p, float v) {
  // (the branch is on the SIGN BIT: -0.0f compares >= 0 but its pattern is INT_MIN, which a signed max never stores)
  if (__float_as_int(v) >= 0) atomicMax(reinterpret_cast<int*>(p), __float_as_int(v));
  else atomicMin(reinterpret_cast<unsigned*>(p), __float_as_uint(v));
}

__device__ __forceinline__ float lna_row_sum(float v) {
  v += __shfl_xor(v, 16);
  v += __shfl_xor(v, 32);
  return v;
}

typedef float lna_f32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ lna_f32x2 lna_pk_fma(lna_f32x2 a, lna_f32x2 b, lna_f32x2 c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ lna_f32x2 lna_pk(float v) { return lna_f32x2{v, v}; }

// GELU: the library's one form (common.h: max(y, 0) - t 2^P(t), one transcendental per value), on TWO values per lane — gfx950 issues
// v_pk_fma_f32 / v_pk_mul_f32 / v_pk_add_f32 at the rate of their scalar forms, and the kernel is bound by VALU issue, not by the
// matrix pipe (docs/kernels/K21_K22_linear_family.md).
__device__ __forceinline__ lna_f32x2 lna_gelu2(lna_f32x2 y) { return fsf_gelu2(y); }

__device__ __forceinline__ lna_f32x2 lna_act2(lna_f32x2 y, int act) {
  if (act == 1) return lna_f32x2{fmaxf(y.x, 0.0f), fmaxf(y.y, 0.0f)};
  if (act == 2) return lna_gelu2(y);
  return y;
}

// ---- K22f / K22h: f16 hi | lo planes (fmt_pick_scale, fmt_split_f16: the scheme of K9c / K9d) -----------------------------------
constexpr unsigned LNA_F16_TAG = 0x4B323266u;  // "K22f": word FMT_HDR_TAG of the f16 weight planes' header

// ---- K22s: segmented max of the activated tile, rows sorted by segment ------------------------------------------------
// Per 16-row group a segmented max-scan along the rows (16 lanes of a DPP row per channel quad), then per run:
//   closed (the segment starts and ends inside the group)  -> its last lane stores the maximum,
//   open at the head and / or the tail                      -> one of the group's two LDS slots (in the weight buffer the last
//                                                              chunk just left free), merged in row order by 128 threads.
// Only a segment that reaches beyond its 128-row block (<= 2 per block) ends in an atomic max; every other segment is stored
// once.  max is exact: the result does not depend on any order.  (A contiguous range of blocks per workgroup with the open
// maximum carried from block to block — atomics only at the range ends — was built first and measured 10 % slower for the
// whole kernel: 768 workgroups each streaming its own region lose to 768 workgroups sweeping one window.)
// The scan runs inside the epilogue's tile loop (four values at a time, right after they are activated): nothing but the
// per-group flags below outlives a tile.
constexpr int LNA_DPP_ROW_SHR = 0x110, LNA_DPP_ROW_SHL = 0x100;

template <int CTRL>
__device__ __forceinline__ float lna_dpp(float old, float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(old), __float_as_int(v), CTRL, 0xf, 0xf, false));
}
template <int CTRL>
__device__ __forceinline__ int lna_dpp_i(int old, int v) { return __builtin_amdgcn_update_dpp(old, v, CTRL, 0xf, 0xf, false); }

constexpr int LNA_SLOT_HEAD_OPEN = 1 << 29, LNA_SLOT_TAIL_OPEN = 1 << 30, LNA_SLOT_SID = (1 << 29) - 1;  // (-1 = empty slot)

struct LnaSegSmem {      // persistent part (behind the per-channel vectors)
  int slot_sid[16];      // segment | LNA_SLOT_HEAD_OPEN | LNA_SLOT_TAIL_OPEN, or -1
};

struct LnaSegCtx {       // per lane, for ONE 16-row group of its wave (built right before the group's tiles: half the live masks)
  bool one_seg;          // (wave-uniform) the whole group is one run
  uint64_t m1, m2, m4, m8;  // lane masks (SGPR pairs): the row 1 / 2 / 4 / 8 above belongs to the same segment
  bool write, to_slot;   // this lane ends a run of a group that holds rows < n; the run is open (its maxima go to an LDS slot)
  int dst;               // float offset of the run's row in seg_out (a closed run) or in the slots — 32 bits: a 64-bit pointer per
                         // lane was spilled and re-read from scratch for every tile
};

template <int RG>
struct LnaSegBlockT {    // what the epilogue needs to build the groups' contexts (RG 16-row groups per wave)
  int sid[RG];       // segment of this lane's row in either group (requested at the top of the block: no exposed latency here)
  int sid_before, sid_after;  // (wave-uniform) segment of the row above the wave's 16 RG rows / below them, -1 where there is none
  int64_t blk_row0;
  int wave;
  float* slots;
  LnaSegSmem* sm;
};
typedef LnaSegBlockT<LNA_RG> LnaSegBlock;

// The scan of one tile's four values, hand-scheduled: a step is ONE instruction per value — `v_max_f32_dpp x, x(row_shr:k), x`, a lane
// whose source lies outside its 16-lane row keeps x (bound_ctrl off) — plus, when the group holds more than one segment, a select on the
// step's lane mask.  As compiled from `fmaxf(x, update_dpp(x, x))` a step was five to six (a copy for the tied old value, the hazard nop,
// v_mov_dpp, a canonicalising v_max of the shuffled operand, the v_max, v_cndmask): the scan was ~1 400 of a wave's ~3 700 VALU
// instructions per row block in a kernel that is bound by VALU issue (profiles/r5_pmc_k22s.txt).  The DPP read-after-VALU-write hazard
// (two wait states; the assembler does not see into the block) is covered by the interleaving: a value's next step comes four
// instructions after its last write, and the block opens with a nop for whatever produced the inputs.
__device__ __forceinline__ float4 lna_seg_scan(const LnaSegCtx& sc, float4 y) {
  float a = y.x, b = y.y, c = y.z, d = y.w;
#define LNA_SCAN_MAX1(K)                                               \
  "v_max_f32_dpp %0, %0, %0 row_shr:" #K " row_mask:0xf bank_mask:0xf\n" \
  "v_max_f32_dpp %1, %1, %1 row_shr:" #K " row_mask:0xf bank_mask:0xf\n" \
  "v_max_f32_dpp %2, %2, %2 row_shr:" #K " row_mask:0xf bank_mask:0xf\n" \
  "v_max_f32_dpp %3, %3, %3 row_shr:" #K " row_mask:0xf bank_mask:0xf\n"
#define LNA_SCAN_MAXSEL(K, M)                                          \
  "v_max_f32_dpp %4, %0, %0 row_shr:" #K " row_mask:0xf bank_mask:0xf\n" \
  "v_max_f32_dpp %5, %1, %1 row_shr:" #K " row_mask:0xf bank_mask:0xf\n" \
  "v_max_f32_dpp %6, %2, %2 row_shr:" #K " row_mask:0xf bank_mask:0xf\n" \
  "v_max_f32_dpp %7, %3, %3 row_shr:" #K " row_mask:0xf bank_mask:0xf\n" \
  "v_cndmask_b32_e64 %0, %0, %4, " M "\n"                              \
  "v_cndmask_b32_e64 %1, %1, %5, " M "\n"                              \
  "v_cndmask_b32_e64 %2, %2, %6, " M "\n"                              \
  "v_cndmask_b32_e64 %3, %3, %7, " M "\n"
  if (sc.one_seg) {  // (wave-uniform) plain prefix maxima, no selects
    asm volatile("s_nop 1\n" LNA_SCAN_MAX1(1) LNA_SCAN_MAX1(2) LNA_SCAN_MAX1(4) LNA_SCAN_MAX1(8)
                 : "+v"(a), "+v"(b), "+v"(c), "+v"(d));
  } else {  // (lanes without a source keep garbage in the scratch values: their mask bits are clear)
    float oa, ob, oc, od;
    asm volatile("s_nop 1\n" LNA_SCAN_MAXSEL(1, "%8") LNA_SCAN_MAXSEL(2, "%9") LNA_SCAN_MAXSEL(4, "%10") LNA_SCAN_MAXSEL(8, "%11")
                 : "+v"(a), "+v"(b), "+v"(c), "+v"(d), "=&v"(oa), "=&v"(ob), "=&v"(oc), "=&v"(od)
                 : "s"(sc.m1), "s"(sc.m2), "s"(sc.m4), "s"(sc.m8));
  }
#undef LNA_SCAN_MAX1
#undef LNA_SCAN_MAXSEL
  return make_float4(a, b, c, d);
}

// one group's segment ids -> scan flags, run ends and their destinations; called after the barrier that frees the slot buffer
// (a workgroup holds eight groups — waves x RG — whatever its shape: two slots each, sixteen in all)
template <int RG>
__device__ __forceinline__ LnaSegCtx lna_seg_prepare(const LnaArgs& a, const LnaSegBlockT<RG>& sb, int rg, int rowl, int grp) {
  LnaSegCtx sc;
  const int g = RG * sb.wave + rg;
  const int64_t grow0 = sb.blk_row0 + 16 * g;
  const int sid = sb.sid[rg];  // (rows past n repeat row n - 1 in every respect: the maxima are unchanged)
  const int up1 = lna_dpp_i<LNA_DPP_ROW_SHR + 1>(-1, sid), up2 = lna_dpp_i<LNA_DPP_ROW_SHR + 2>(-1, sid);
  const int up4 = lna_dpp_i<LNA_DPP_ROW_SHR + 4>(-1, sid), up8 = lna_dpp_i<LNA_DPP_ROW_SHR + 8>(-1, sid);
  const int dn1 = lna_dpp_i<LNA_DPP_ROW_SHL + 1>(-1, sid);
  sc.m1 = __builtin_amdgcn_ballot_w64(up1 == sid); sc.m2 = __builtin_amdgcn_ballot_w64(up2 == sid);  // (ids >= 0: -1 = no such lane)
  sc.m4 = __builtin_amdgcn_ballot_w64(up4 == sid); sc.m8 = __builtin_amdgcn_ballot_w64(up8 == sid);
  sc.one_seg = __builtin_amdgcn_readfirstlane(sid) == __builtin_amdgcn_readlane(sid, 15);  // sorted: first == last
  sc.write = sc.to_slot = false;
  sc.dst = 0;
  if (grow0 < a.n && (rowl == 15 || dn1 != sid)) {  // (a group past the last row forms no run: its slots stay empty)
    sc.write = true;
    // a run is open at the head iff it is the group's first run and the row above the group belongs to the same segment (ids are
    // sorted), open at the tail iff it is the last run and the row below does: no look-up of the segment's bounds
    const int first = __builtin_amdgcn_readfirstlane(sid), last = __builtin_amdgcn_readlane(sid, 15);
    const int above = rg == 0 ? sb.sid_before : __builtin_amdgcn_readlane(sb.sid[rg > 0 ? rg - 1 : 0], 15);
    const int below = rg == RG - 1 ? sb.sid_after : __builtin_amdgcn_readfirstlane(sb.sid[rg + 1 < RG ? rg + 1 : RG - 1]);
    const bool head_open = sid == first && above == first, tail_open = sid == last && below == last;
    if (!head_open && !tail_open) {
      sc.dst = sid * (int)a.seg_out_stride;
    } else {
      const int slot = 2 * g + (head_open ? 0 : 1);
      if (grp == 0) sb.sm->slot_sid[slot] = sid | (head_open ? LNA_SLOT_HEAD_OPEN : 0) | (tail_open ? LNA_SLOT_TAIL_OPEN : 0);
      sc.to_slot = true;
      sc.dst = slot * 128;
    }
  }
  return sc;
}

// after every wave has parked its open runs: merge them in row order (128 threads, one per channel).  A segment whose parts all
// lie in this 128-row block (its first slot is closed at the head, its last at the tail) is stored plainly; one that reaches into
// a neighbouring block — some other workgroup's — is combined by atomic max: at most two per block, fire-and-forget.
__device__ __forceinline__ void lna_seg_merge(const LnaArgs& a, const float* slots, const LnaSegSmem* sm) {
  __syncthreads();
  if (threadIdx.x < 128) {
    const int ch = threadIdx.x;
    int cs = -1;  // segment | LNA_SLOT_HEAD_OPEN (it began above this block)
    float cv = -INFINITY;
    auto flush = [&](int tag, float v, bool complete) {
      if (ch >= a.c) return;
      float* p = a.seg_out + (int64_t)(tag & LNA_SLOT_SID) * a.seg_out_stride + ch;
      if (complete && !(tag & LNA_SLOT_HEAD_OPEN)) *p = v;
      else lna_atomic_max(p, v);
    };
    for (int s = 0; s < 16; ++s) {
      const int ss = sm->slot_sid[s];
      if (ss < 0) continue;
      const float v = slots[s * 128 + ch];
      if (cs >= 0 && (ss & LNA_SLOT_SID) == (cs & LNA_SLOT_SID)) cv = fmaxf(cv, v);
      else {  // (an open segment always continues in the next occupied slot; kept general)
        if (cs >= 0) flush(cs, cv, false);
        cs = ss & (LNA_SLOT_SID | LNA_SLOT_HEAD_OPEN);
        cv = v;
      }
      if (!(ss & LNA_SLOT_TAIL_OPEN)) {  // the segment ends in this group
        flush(cs, cv, true);
        cs = -1;
      }
    }
    if (cs >= 0) flush(cs, cv, false);  // continues below this block
  }
}

// epilogue of one row block: lane (row, g) holds channels ch_base + 16 t + 4 g + r of its row
// bias | gamma | beta of the 128-channel slice at ch_base -> LDS (defaults 0 | 1 | 0 where absent or beyond c)
__device__ __forceinline__ void lna_stage_vectors(const LnaArgs& a, int ch_base, float* vec) {
  for (int t = threadIdx.x; t < 384; t += blockDim.x) {
    const int which = t >> 7, ch = ch_base + (t & 127);
    const float* src = which == 0 ? a.bias : (a.norm != 0 ? (which == 1 ? a.gamma : a.beta) : nullptr);
    vec[t] = (src && (t & 127) < a.slice_w && ch < a.c) ? src[ch] : (which == 1 ? 1.0f : 0.0f);
  }
  __syncthreads();
}

// `vec` = this slice's bias | gamma | beta, 128 floats each, staged in LDS once per workgroup: as ordinary global loads in
// here every one of them was followed by the `vmcnt(0)` hipcc emits at the first use of a load beside an LDS-DMA — 24-48
// serialized L2 round trips per row block (and a drain of the next block's prefetch each time).
template <int T, bool SEG = false, int NORM_CT = -1, int ACT_CT = -1, int RG = LNA_RG>  // SEG: the activated values also go through the segmented
// max-scan; NORM_CT / ACT_CT >= 0: norm and activation fixed at compile time (the K22s variants: their epilogue is already twice
// the code, and the run-time switches of the plain kernel would double it again)
__device__ __forceinline__ void lna_epilogue(const LnaArgs& a, lna_f32x4 (&acc)[RG][T], int64_t row0, int ch_base, int rowl,
                                             int grp, const float* vec, const LnaSegBlockT<RG>* sb = nullptr) {
  const float inv_c = 1.0f / (float)a.norm_w;
  // the arithmetic below runs on pairs (v_pk_*_f32): the same IEEE operations per value as the scalar form, half the instructions
  auto lo = [](const lna_f32x4& v) { return lna_f32x2{v[0], v[1]}; };
  auto hi = [](const lna_f32x4& v) { return lna_f32x2{v[2], v[3]}; };
  auto put = [](lna_f32x4& v, lna_f32x2 l, lna_f32x2 h) { v[0] = l.x; v[1] = l.y; v[2] = h.x; v[3] = h.y; };
#pragma unroll
  for (int rg = 0; rg < RG; ++rg) {
    const int64_t row = row0 + 16 * rg + rowl;
    float mean = 0.0f, rstd = 1.0f;
    LnaSegCtx sc;
    int g4 = 4 * grp;  // this lane's channel offset inside a tile
    if constexpr (SEG) {
      sc = lna_seg_prepare<RG>(a, *sb, rg, rowl, grp);
      // (opaque: with the scan's live state on top, the compiler otherwise hoists the 64-bit per-lane store offsets of all tiles out
      // of the block loop, spills them, and re-reads one from scratch in front of every tile's stores)
      asm volatile("" : "+v"(g4));
    }
    if (a.bias) {
#pragma unroll
      for (int t = 0; t < T; ++t) {
        const float4 b = *reinterpret_cast<const float4*>(vec + 16 * t + 4 * grp);  // (0 beyond c)
        put(acc[rg][t], lo(acc[rg][t]) + lna_f32x2{b.x, b.y}, hi(acc[rg][t]) + lna_f32x2{b.z, b.w});
      }
    }
    if (a.row_add) {  // all loads of the row first, then the adds: one wait instead of one per tile
      const int64_t row_c = row0 + 16 * rg + rowl;
      const float* add = a.row_add + a.row_add_index[row_c < a.n ? row_c : a.n - 1] * a.row_add_stride;
      constexpr int TB = T < 4 ? T : 4;  // four loads in flight per wait
#pragma unroll
      for (int t0 = 0; t0 < T; t0 += TB) {
        float4 b[TB];
#pragma unroll
        for (int t = 0; t < TB; ++t) {
          const int lc0 = 16 * (t0 + t) + 4 * grp, ch0 = ch_base + lc0;
          b[t] = *reinterpret_cast<const float4*>(add + (lc0 < a.slice_w && ch0 < a.c ? ch0 : 0));
        }
#pragma unroll
        for (int t = 0; t < TB; ++t) {
          if (16 * (t0 + t) + 4 * grp < a.slice_w && ch_base + 16 * (t0 + t) + 4 * grp < a.c)
            put(acc[rg][t0 + t], lo(acc[rg][t0 + t]) + lna_f32x2{b[t].x, b[t].y}, hi(acc[rg][t0 + t]) + lna_f32x2{b[t].z, b[t].w});
        }
      }
    }
    if ((NORM_CT >= 0 ? NORM_CT : a.norm) == 1) {  // LayerNorm over the c channels (channels >= c are exactly 0: zero weights, no bias)
      lna_f32x2 s2 = lna_pk(0.0f);
#pragma unroll
      for (int t = 0; t < T; ++t) s2 = (s2 + lo(acc[rg][t])) + hi(acc[rg][t]);
      mean = lna_row_sum(s2.x + s2.y) * inv_c;
      const lna_f32x2 m2 = lna_pk(mean);
      lna_f32x2 q2 = lna_pk(0.0f);
#pragma unroll
      for (int t = 0; t < T; ++t) {
        const bool live = 16 * t + 4 * grp < a.slice_w && ch_base + 16 * t + 4 * grp < a.c;  // (widths are multiples of 4)
        const lna_f32x2 dl = live ? lo(acc[rg][t]) - m2 : lna_pk(0.0f), dh = live ? hi(acc[rg][t]) - m2 : lna_pk(0.0f);
        q2 = lna_pk_fma(dl, dl, q2);
        q2 = lna_pk_fma(dh, dh, q2);
      }
      rstd = rsqrtf(lna_row_sum(q2.x + q2.y) * inv_c + a.eps);
    }
    if (row < a.n || SEG) {
      float* orow = a.out + row * a.out_stride;
      const lna_f32x2 m2 = lna_pk(mean), r2 = lna_pk(rstd);
#pragma unroll
      for (int t = 0; t < T; ++t) {
        const int ch0 = ch_base + 16 * t + g4;
        if (16 * t + 4 * grp < a.slice_w && ch_base + 16 * t + 4 * grp < a.c) {
          const float4 g = *reinterpret_cast<const float4*>(vec + 128 + 16 * t + 4 * grp);  // (1 / 0 without a norm)
          const float4 b = *reinterpret_cast<const float4*>(vec + 256 + 16 * t + 4 * grp);
          const lna_f32x2 yl = lna_act2((lo(acc[rg][t]) - m2) * r2 * lna_f32x2{g.x, g.y} + lna_f32x2{b.x, b.y}, ACT_CT >= 0 ? ACT_CT : a.act);
          const lna_f32x2 yh = lna_act2((hi(acc[rg][t]) - m2) * r2 * lna_f32x2{g.z, g.w} + lna_f32x2{b.z, b.w}, ACT_CT >= 0 ? ACT_CT : a.act);
          const float4 y = make_float4(yl.x, yl.y, yh.x, yh.y);
          if (!SEG || (a.out && row < a.n)) *reinterpret_cast<float4*>(orow + ch0) = y;
          if constexpr (SEG) {
            const float4 mx = lna_seg_scan(sc, y);  // (a group past the last row scans copies of row n - 1 and writes nothing)
            if (sc.write) {
              if (sc.to_slot) *reinterpret_cast<float4*>(sb->slots + (sc.dst + 16 * t + g4)) = mx;
              else *reinterpret_cast<float4*>(a.seg_out + (sc.dst + 16 * t + g4)) = mx;
            }
          }
        }
      }
    }
  }
}

// ---- K22f (XM = 2): the two steps of a k chunk that the fused K21 + K22s kernel (csrc/sir_linear.hip) shares ------------------------
// A row's chunk is scaled by a power of two s with s * max|x| in [2^13, 2^14) and split into f16 hi + lo (22 bits relative to the
// maximum — the arithmetic of K9d / K22h).  The scale may only FALL from chunk to chunk (it follows the running maximum of the row, so a
// row is held to 22 bits of ITS maximum, like a whole-row scale would); when it falls, the row's accumulators, which are kept in the
// unit s * s_w, are multiplied by new / old — a power of two, exact.  The first chunk's scale is capped (xs_cap) where a per-row addend
// sits in the accumulators, which it enters multiplied by s * s_w.
template <int RG, int T>
__device__ __forceinline__ void lna_xf_scale_split(const float (&xc)[RG][8], int kc, float (&xs_cur)[RG], float (&xinv)[RG], lna_u32x4 (&xh)[RG],
                                                   lna_u32x4 (&xl)[RG], lna_f32x4 (&acc)[RG][T], float w_scale, float xs_cap, float xs_cap_inv,
                                                   bool has_addend) {
  float ratio[RG];
  bool changed = false;
#pragma unroll
  for (int rg = 0; rg < RG; ++rg) {
    unsigned mb = __float_as_uint(xc[rg][0]) & 0x7fffffffu;  // (bit patterns of |x| order like the values; NaN / inf end up largest)
#pragma unroll
    for (int e = 1; e < 8; ++e) mb = max(mb, __float_as_uint(xc[rg][e]) & 0x7fffffffu);
    const auto r16 = __builtin_amdgcn_permlane16_swap(mb, mb, false, false);  // the four lanes of a row: lane ^ 16, lane ^ 32
    mb = max(r16[0], r16[1]);
    const auto r32 = __builtin_amdgcn_permlane32_swap(mb, mb, false, false);
    mb = max(r32[0], r32[1]);
    float s_new, inv_new;
    fmt_pick_scale(__uint_as_float(mb), s_new, inv_new);
    if (kc == 0) {
      if (mb == 0u || s_new > xs_cap) { s_new = xs_cap; inv_new = xs_cap_inv; }
      ratio[rg] = s_new * w_scale;
      changed |= has_addend;  // (the accumulators hold the addend, unit 1, or zeros)
    } else {
      if (mb == 0u || s_new > xs_cur[rg]) { s_new = xs_cur[rg]; inv_new = xinv[rg]; }
      ratio[rg] = s_new * xinv[rg];  // (1 where nothing changed)
      changed |= s_new != xs_cur[rg];
    }
    xs_cur[rg] = s_new;
    xinv[rg] = inv_new;
    fmt_split_f16(xc[rg], s_new, xh[rg], xl[rg]);
  }
  if (__builtin_amdgcn_ballot_w64(changed) != 0) {  // (wave-uniform: rare after the first chunk)
#pragma unroll
    for (int rg = 0; rg < RG; ++rg)
#pragma unroll
      for (int t = 0; t < T; ++t) acc[rg][t] = acc[rg][t] * ratio[rg];
  }
}

// the chunk's products on f16 hi | lo planes (`wc`: the chunk's weight fragments in LDS, [T][2 planes][64 lanes] x 16 B).  Two channel
// tiles x RG row groups = independent accumulators per product term: consecutive MFMAs never hit the same accumulator
template <int RG, int T>
__device__ __forceinline__ void lna_mfma_f16_chunk(const uint4* wc, int lane, const lna_u32x4 (&xh)[RG], const lna_u32x4 (&xl)[RG],
                                                   lna_f32x4 (&acc)[RG][T]) {
#pragma unroll
  for (int t = 0; t < T; t += 2) {
    lna_f16x8 wfr[2][2];
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) {
      const uint4* wf = wc + ((t + tt) * 2) * 64 + lane;
#pragma unroll
      for (int pl = 0; pl < 2; ++pl) wfr[tt][pl] = __builtin_bit_cast(lna_f16x8, wf[64 * pl]);
    }
    // (weight plane, x plane): lo hi, hi lo, hi hi — small terms first
    constexpr int TERM_W[3] = {1, 0, 0};
    constexpr int TERM_X[3] = {0, 1, 0};
#pragma unroll
    for (int term = 0; term < 3; ++term)
#pragma unroll
      for (int tt = 0; tt < 2; ++tt)
#pragma unroll
        for (int rg = 0; rg < RG; ++rg) {
          const lna_u32x4 xb = TERM_X[term] == 0 ? xh[rg] : xl[rg];
          acc[rg][t + tt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wfr[tt][TERM_W[term]], __builtin_bit_cast(lna_f16x8, xb), acc[rg][t + tt],
                                                                   0, 0, 0);
        }
  }
}

}  // namespace fsf
