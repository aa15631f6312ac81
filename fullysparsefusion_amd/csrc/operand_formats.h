// The two operand formats the matrix-core product kernels feed their MFMAs, defined once (tests/product_budget.py derives every
// per-element error budget from them):
//   * the exact bf16 three-way split hi + mid + lo by truncation, six cross terms (K22, K9b, K10p);
//   * f16 hi | lo planes of x * s, s a power of two with s * amax in [2^13, 2^14) (K9c / K9d, K9b-XP, K22f, K22h), and the 256-byte
//     header in front of a layer's weight planes in that form.
#pragma once
#include "common.h"

namespace fsf {

template <int N>
using fmt_u32v = unsigned __attribute__((ext_vector_type(N)));
template <int N>
using fmt_f16v = _Float16 __attribute__((ext_vector_type(N)));

// The header of a layer's f16 weight planes: the fragments start FMT_HDR_BYTES behind it.
constexpr int FMT_HDR_BYTES = 256;
constexpr int FMT_HDR_U4 = FMT_HDR_BYTES / 16;  // ... in 16-byte fragments
constexpr int FMT_HDR_INV_SCALE = 0;            // word 0: 1 / s_w (f32)
constexpr int FMT_HDR_SCALE = 1;                // word 1: s_w (f32)
constexpr int FMT_HDR_AMAX_BITS = 2;            // word 2: the bit pattern of max |w| over the layer (fsf_weight_layer_absmax)
constexpr int FMT_HDR_TAG = 3;                  // word 3: the format's tag where the consumer checks one (K22f / K22h: LNA_F16_TAG)

// power of two s with s * amax in [2^13, 2^14) (s = 2^0 for amax = 0), inv = 1 / s: both exact, and both stay normal fp32 numbers for
// every finite amax (the exponent is clamped at -113: s <= 2^126)
__device__ __forceinline__ void fmt_pick_scale(float amax, float& s, float& inv) {
  int e = (int)((__float_as_uint(amax) >> 23) & 0xffu) - 127;
  e = amax > 0.0f ? (e < -113 ? -113 : e) : 13;
  s = __uint_as_float((unsigned)(13 - e + 127) << 23);
  inv = __uint_as_float((unsigned)(e - 13 + 127) << 23);
}

// exact three-way split of N floats into bf16 planes (two bf16 per dword, element 2j in the low half): each piece is the next 8
// significant bits, by truncation, the remainders formed in fp32 — nothing is rounded away
template <int N>
__device__ __forceinline__ void fmt_split_bf16(const float (&v)[N], fmt_u32v<N / 2>& hi, fmt_u32v<N / 2>& mid, fmt_u32v<N / 2>& lo) {
#pragma unroll
  for (int j = 0; j < N / 2; ++j) {
    const float a = v[2 * j], b = v[2 * j + 1];
    const float ah = __uint_as_float(__float_as_uint(a) & 0xffff0000u), bh = __uint_as_float(__float_as_uint(b) & 0xffff0000u);
    const float ar = __fsub_rn(a, ah), br = __fsub_rn(b, bh);
    const float am = __uint_as_float(__float_as_uint(ar) & 0xffff0000u), bm = __uint_as_float(__float_as_uint(br) & 0xffff0000u);
    const float al = __fsub_rn(ar, am), bl = __fsub_rn(br, bm);
    hi[j] = __builtin_amdgcn_perm(__float_as_uint(bh), __float_as_uint(ah), 0x07060302u);
    mid[j] = __builtin_amdgcn_perm(__float_as_uint(bm), __float_as_uint(am), 0x07060302u);
    lo[j] = __builtin_amdgcn_perm(__float_as_uint(bl), __float_as_uint(al), 0x07060302u);
  }
}

// f16 hi | lo of N floats at the scale s: hi = rn_f16(x s), lo = rn_f16(x s - hi): |x s - hi - lo| <= max(2^-22 |x s|, 2^-25), no f16
// range hazard for any finite input when s comes from fmt_pick_scale of a maximum over x
template <int N>
__device__ __forceinline__ void fmt_split_f16(const float (&v)[N], float s, fmt_u32v<N / 2>& hi, fmt_u32v<N / 2>& lo) {
  fmt_f16v<N> h, l;
#pragma unroll
  for (int e = 0; e < N; ++e) {
    const float xs = __fmul_rn(v[e], s);
    h[e] = (_Float16)xs;
    l[e] = (_Float16)__fsub_rn(xs, (float)h[e]);
  }
  hi = __builtin_bit_cast(fmt_u32v<N / 2>, h);
  lo = __builtin_bit_cast(fmt_u32v<N / 2>, l);
}

// max |w| over a layer's n weights into word FMT_HDR_AMAX_BITS of the header at `hdr`, the other FMT_HDR_BYTES - 4 bytes cleared
// (operand_formats.hip).  The prepare kernel that follows on the stream picks the layer's ONE scale from that word.
int fsf_weight_layer_absmax(const float* w, int64_t n, void* hdr, hipStream_t stream);

}  // namespace fsf
