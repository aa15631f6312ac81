// K41: the nuScenes detection protocol (detection_cvpr_2019) on the device — see include/fsf_hip.h and docs/kernels/K41_det_eval.md.
//   fsf_det_eval_compute: accumulated predictions + ground truth of a validation pass -> centre-distance matches, precision / confidence /
//   true-positive-error curves, AP, TP errors, mAP and NDS, in one result block.  Launches, in stream order:
//     prep          keys of sort A = (class << 32 | monotone u32 of the score), the effective GT class, the GT offsets per sample
//     sort A        stable ascending radix sort: a class's range read BACKWARDS is the specification's processing order (descending score,
//                   the later position first among equal scores)
//     order         keys of sort B = (sample, class) of the predictions taken in that backwards order; the class offsets
//     sort B        stable: each (sample, class) segment's predictions contiguous and in processing order
//     bounds        the segment offsets
//     K41a match    one wave per (segment, threshold): predictions serially, lanes stride over the sample's GT, shuffle-reduced minimum of
//                   (distance, GT position); the five errors at the TP threshold
//     K41b curves   one workgroup per (class, threshold): tp prefix counts and the NaN-skipping fp64 prefix sums by a tile loop with a carry
//                   (fixed order, no float atomics), then the 101-point interpolations with np.interp's semantics
//     K41c summary  one workgroup: AP, TP errors, mAP, the mean errors, NDS
// Arithmetic is fp64 with every product, sum and quotient rounded on its own (the library is built with contraction off; the distance is
// written with __dmul_rn / __dadd_rn all the same: a contracted dx*dx + dy*dy moves ties at a strict threshold), in the order of
// mmdet3d_plugin/core/det_eval.py.
#include "common.h"
#include "radix_sort.h"

namespace fsf {

constexpr int DE_PTS = 101;          // recall points, np.linspace(0, 1, 101)
constexpr int DE_ERRS = 5;           // trans, scale, orient, vel, attr
constexpr int DE_BOX = 9;            // x, y, z, w, l, h, yaw, vx, vy
constexpr int DE_CURVE_THREADS = 1024;
constexpr double DE_PI = 3.14159265358979323846;

struct DetEvalLayout {
  RadixScratch sort;
  uint32_t* ord;       // [P]   original index of the prediction at position a of sort A
  int32_t* cls_off;    // [C+2] ranges of sort A per class; class C = ignored rows
  int32_t* seg_off;    // [S*(C+1)+1] ranges of sort B per (sample, class)
  int32_t* gt_off;     // [S+1]
  int32_t* gt_cls;     // [G]   effective class of a GT row, -1 = ignored
  uint8_t* taken;      // [T*G]
  int32_t* match_s;    // [T*P] matched GT per position of sort A
  double* errs;        // [5*P] per position of sort A, written for the matches of the TP threshold
  uint32_t* tpcum;     // [T*P] inclusive tp count per position of sort A
  double* mconf;       // [P]   confidence of a class's m-th match at cls_off[c] + m
  double* cm;          // [5*P] cummean of a class's m-th match
  double* stats;       // [C*T*8] ntp, no_predictions, npos, npred, all-NaN flags of the five errors (as bits)
  DetEvalLayout(FsfArena& ar, int64_t P, int64_t G, int64_t S, int64_t C, int64_t T)
      : sort(ar, P), ord(ar.take<uint32_t>(P)), cls_off(ar.take<int32_t>(C + 2)), seg_off(ar.take<int32_t>(S * (C + 1) + 1)),
        gt_off(ar.take<int32_t>(S + 1)), gt_cls(ar.take<int32_t>(G)), taken(ar.take<uint8_t>(T * G)), match_s(ar.take<int32_t>(T * P)),
        errs(ar.take<double>(DE_ERRS * P)), tpcum(ar.take<uint32_t>(T * P)), mconf(ar.take<double>(P)), cm(ar.take<double>(DE_ERRS * P)),
        stats(ar.take<double>(C * T * 8)) {}
};

struct DeArgs {
  int64_t P, G;
  int S, C, T, t_tp, first;
  double min_precision, ap_weight;
  double ths[FSF_DET_EVAL_MAX_THRESHOLDS];
  int use_range;
  int flags[FSF_DET_EVAL_MAX_CLASSES];     // bit 0: orientation period pi; bit 1 + e: the class does not define error e
  double range[FSF_DET_EVAL_MAX_CLASSES];  // class_range
};

// f32 bits -> u32 with the same order as the floats (-0 < +0, NaN of either sign at an end)
__device__ __forceinline__ uint32_t de_mono(float f) {
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ double de_dist(double ax, double ay, double bx, double by) {
  const double dx = ax - bx, dy = ay - by;
  return __dsqrt_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)));
}

// the class a row counts for: its label when that names a class and the row lies inside the class's range, else `none`
__device__ __forceinline__ int de_class(const DeArgs& a, int label, const float* row, int none) {
  if (label < 0 || label >= a.C) return none;
  if (a.use_range) {
    const double r = de_dist((double)row[0], (double)row[1], 0.0, 0.0);
    if (r > a.range[label]) return none;
  }
  return label;
}

// offsets of the runs of a non-decreasing key sequence: off[k] = first i with key(i) >= k, for k in [0, nkeys]
template <class Key>
__device__ __forceinline__ void de_bounds(int64_t i, int64_t n, int64_t nkeys, Key key, int32_t* off) {
  const int64_t k0 = i > 0 ? key(i - 1) : -1;
  int64_t k1 = i < n ? key(i) : nkeys;
  if (k1 > nkeys) k1 = nkeys;
  for (int64_t k = k0 + 1; k <= k1; ++k) off[k] = (int32_t)i;
}

__global__ void __launch_bounds__(256)
    de_prep_kernel(DeArgs a, const float* __restrict__ pred, const float* __restrict__ score, const int32_t* __restrict__ plabel,
                   const float* __restrict__ gt, const int32_t* __restrict__ glabel, const int32_t* __restrict__ gsample,
                   uint64_t* __restrict__ keys, uint32_t* __restrict__ vals,
                   int32_t* __restrict__ match_out, int32_t* __restrict__ gt_cls, int32_t* __restrict__ gt_off) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x, tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (int64_t p = tid; p < a.P; p += stride) {
    const int c = de_class(a, plabel[p], pred + p * DE_BOX, a.C);
    keys[p] = ((uint64_t)c << 32) | de_mono(score[p]);
    vals[p] = (uint32_t)p;
    for (int t = 0; t < a.T; ++t) match_out[t * a.P + p] = -1;
  }
  for (int64_t g = tid; g < a.G; g += stride) gt_cls[g] = de_class(a, glabel[g], gt + g * DE_BOX, -1);
  for (int64_t g = tid; g <= a.G; g += stride)
    de_bounds(g, a.G, a.S, [&](int64_t i) { return (int64_t)(gsample[i] < 0 ? 0 : gsample[i]); }, gt_off);
}

// position q of the whole backwards order <-> position P - 1 - q of sort A
__global__ void __launch_bounds__(256)
    de_order_kernel(DeArgs a, const uint64_t* __restrict__ keys_sorted, const uint32_t* __restrict__ vals_sorted,
                    const int32_t* __restrict__ psample, uint64_t* __restrict__ keys2, uint32_t* __restrict__ vals2,
                    uint32_t* __restrict__ ord, int32_t* __restrict__ cls_off) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x, tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (int64_t q = tid; q < a.P; q += stride) {
    const int64_t pos = a.P - 1 - q;
    const uint32_t p = vals_sorted[pos];
    int s = psample[p];
    s = s < 0 ? 0 : (s >= a.S ? a.S - 1 : s);
    keys2[q] = (uint64_t)s * (uint64_t)(a.C + 1) + (keys_sorted[pos] >> 32);
    vals2[q] = (uint32_t)pos;
    ord[pos] = p;
  }
  for (int64_t i = tid; i <= a.P; i += stride)
    de_bounds(i, a.P, (int64_t)a.C + 1, [&](int64_t j) { return (int64_t)(keys_sorted[j] >> 32); }, cls_off);
}

__global__ void __launch_bounds__(256)
    de_seg_bounds_kernel(DeArgs a, const uint64_t* __restrict__ keys2_sorted, int32_t* __restrict__ seg_off) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x, tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (int64_t i = tid; i <= a.P; i += stride)
    de_bounds(i, a.P, (int64_t)a.S * (a.C + 1), [&](int64_t j) { return (int64_t)keys2_sorted[j]; }, seg_off);
}

__device__ __forceinline__ int64_t de_clamp(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

// Python's float %: the sign of the (positive) period
__device__ __forceinline__ double de_pymod(double v, double period) {
  double r = fmod(v, period);
  if (r != 0.0 && r < 0.0) r += period;
  return r;
}

// K41a: work item = (sample, class, threshold), one wave each
__global__ void __launch_bounds__(256)
    de_match_kernel(DeArgs a, const float* __restrict__ pred, const int32_t* __restrict__ pattr, const float* __restrict__ gt,
                    const int32_t* __restrict__ gattr, const int32_t* __restrict__ gt_cls,
                    const int32_t* __restrict__ gt_off, const int32_t* __restrict__ seg_off, const uint32_t* __restrict__ seg_order,
                    const uint32_t* __restrict__ ord, uint8_t* __restrict__ taken, int32_t* __restrict__ match_out,
                    int32_t* __restrict__ match_s, double* __restrict__ errs) {
  const int lane = fsf_lane();
  const int64_t items = (int64_t)a.S * a.C * a.T;
  for (int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); w < items; w += (int64_t)gridDim.x * 4) {
    const int t = (int)(w % a.T);
    const int64_t sc = w / a.T;
    const int c = (int)(sc % a.C);
    const int64_t s = sc / a.C, seg = s * (a.C + 1) + c;
    const int64_t plo = de_clamp(seg_off[seg], 0, a.P), phi = de_clamp(seg_off[seg + 1], plo, a.P);
    if (plo == phi) continue;
    const int64_t glo = de_clamp(gt_off[s], 0, a.G), ghi = de_clamp(gt_off[s + 1], glo, a.G);
    const double th = a.ths[t];
    uint8_t* tk = taken + (int64_t)t * a.G;
    for (int64_t k = plo; k < phi; ++k) {
      const int64_t pos = seg_order[k] < a.P ? seg_order[k] : 0;
      const int64_t p = ord[pos] < a.P ? ord[pos] : 0;
      const float* pr = pred + p * DE_BOX;
      const double px = (double)pr[0], py = (double)pr[1];
      double bd = __builtin_inf();
      int bj = 0x7FFFFFFF;
      for (int64_t j = glo + lane; j < ghi; j += 64) {
        if (gt_cls[j] != c || tk[j]) continue;
        const double d = de_dist((double)gt[j * DE_BOX], (double)gt[j * DE_BOX + 1], px, py);
        if (d < bd) {  // strict: the lane's first GT wins a tie
          bd = d;
          bj = (int)j;
        }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {  // minimum of (distance, GT position): the first GT wins a tie whatever the lane
        const double od = __shfl_xor(bd, o);
        const int oj = __shfl_xor(bj, o);
        if (od < bd || (od == bd && oj < bj)) {
          bd = od;
          bj = oj;
        }
      }
      const bool hit = bj != 0x7FFFFFFF && bd < th;  // strict: a distance equal to the threshold is a miss
      // the lane that tests GT j is the one that marks it: a taken byte is read and written by one thread only
      if (hit && ((bj - glo) & 63) == lane) tk[bj] = 1;
      if (lane == 0) {
        match_out[(int64_t)t * a.P + p] = hit ? bj : -1;
        match_s[(int64_t)t * a.P + pos] = hit ? bj : -1;
        if (hit && t == a.t_tp) {
          const float* g = gt + (int64_t)bj * DE_BOX;
          errs[0 * a.P + pos] = bd;
          double inter = 1.0, vg = 1.0, vp = 1.0;
          for (int d = 3; d < 6; ++d) {
            const double sg = (double)g[d], sp = (double)pr[d];
            inter *= sg < sp ? sg : sp;  // np.minimum
            vg *= sg;
            vp *= sp;
          }
          errs[1 * a.P + pos] = 1.0 - inter / (vg + vp - inter);
          const double period = (a.flags[c] & 1) ? DE_PI : 2.0 * DE_PI;
          double diff = de_pymod((double)g[6] - (double)pr[6] + period / 2.0, period) - period / 2.0;
          if (diff > DE_PI) diff -= 2.0 * DE_PI;
          errs[2 * a.P + pos] = fabs(diff);
          errs[3 * a.P + pos] = de_dist((double)g[7], (double)g[8], (double)pr[7], (double)pr[8]);
          const int ga = gattr[bj];
          errs[4 * a.P + pos] = ga < 0 ? __builtin_nan("") : (ga == pattr[p] ? 0.0 : 1.0);
        }
      }
    }
  }
}

// what K41b scans along a class: the tp flag, and per error the finite count and sum over the matches
struct DeAcc {
  uint32_t tp;
  uint32_t cnt[DE_ERRS];
  double sum[DE_ERRS];
};
template <bool ERR>
__device__ __forceinline__ void de_add(DeAcc& x, const DeAcc& y) {  // x = y + x (y precedes x)
  x.tp += y.tp;
  if (ERR) {
#pragma unroll
    for (int e = 0; e < DE_ERRS; ++e) {
      x.cnt[e] += y.cnt[e];
      x.sum[e] = y.sum[e] + x.sum[e];
    }
  }
}
template <bool ERR>
__device__ __forceinline__ DeAcc de_shfl_up(const DeAcc& v, int o) {
  DeAcc r;
  r.tp = __shfl_up(v.tp, o);
  if (ERR) {
#pragma unroll
    for (int e = 0; e < DE_ERRS; ++e) {
      r.cnt[e] = __shfl_up(v.cnt[e], o);
      r.sum[e] = __shfl_up(v.sum[e], o);
    }
  }
  return r;
}

// inclusive scan of one tile (one value per thread) on top of `carry`, which becomes the tile's last inclusive value: the wave scans by
// shuffles, the 16 wave totals serially, always in the same order
template <bool ERR>
__device__ __forceinline__ DeAcc de_tile_scan(DeAcc v, DeAcc& carry, DeAcc* wave_tot) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const DeAcc u = de_shfl_up<ERR>(v, o);
    if (lane >= o) de_add<ERR>(v, u);
  }
  __syncthreads();  // (wave_tot is reused from the tile before)
  if (lane == 63) wave_tot[wave] = v;
  __syncthreads();
  DeAcc base = carry;
  for (int w = 0; w < wave; ++w) {
    DeAcc x = wave_tot[w];
    de_add<ERR>(x, base);
    base = x;
  }
  de_add<ERR>(v, base);
  DeAcc last = carry;
  for (int w = 0; w < DE_CURVE_THREADS / 64; ++w) {
    DeAcc x = wave_tot[w];
    de_add<ERR>(x, last);
    last = x;
  }
  carry = last;
  return v;
}

struct DeCurveView {  // a class's curve at one threshold, by position q of the processing order
  const uint32_t* tpcum;
  const uint32_t* ord;
  const float* score;
  int64_t hi;  // q <-> position hi - 1 - q of sort A
  double npos;
  __device__ double tp(int64_t q) const { return (double)tpcum[hi - 1 - q]; }
  __device__ double rec(int64_t q) const { return tp(q) / npos; }
  __device__ double prec(int64_t q) const { return tp(q) / (double)(q + 1); }
  __device__ double conf(int64_t q) const { return (double)score[ord[hi - 1 - q]]; }
};

template <bool ERR>
__device__ void de_curve_tiles(const DeArgs& a, int t, int64_t lo, int64_t n, const int32_t* match_s, const double* errs,
                               const float* score, const uint32_t* ord, uint32_t* tpcum, double* mconf, double* cm, DeAcc& carry,
                               DeAcc* wave_tot) {
  const int64_t hi = lo + n;
  for (int64_t q0 = 0; q0 < n; q0 += DE_CURVE_THREADS) {
    const int64_t q = q0 + threadIdx.x, pos = hi - 1 - q;
    const bool valid = q < n;
    DeAcc v;
    v.tp = valid && match_s[(int64_t)t * a.P + pos] >= 0 ? 1u : 0u;
#pragma unroll
    for (int e = 0; e < DE_ERRS; ++e) {
      const double x = (ERR && v.tp) ? errs[e * a.P + pos] : __builtin_nan("");
      v.cnt[e] = x == x ? 1u : 0u;
      v.sum[e] = x == x ? x : 0.0;
    }
    const bool is_tp = v.tp != 0;
    v = de_tile_scan<ERR>(v, carry, wave_tot);
    if (valid) tpcum[(int64_t)t * a.P + pos] = v.tp;
    if (ERR && is_tp) {
      const int64_t slot = lo + v.tp - 1;
      mconf[slot] = (double)score[ord[pos]];
#pragma unroll
      for (int e = 0; e < DE_ERRS; ++e) cm[e * a.P + slot] = v.cnt[e] ? v.sum[e] / (double)v.cnt[e] : 0.0;
    }
  }
}

// K41b: one workgroup per (class, threshold).  curves f64 [C, 2 T + 5, 101]: precision per threshold, confidence per threshold, the five
// error curves of the TP threshold
__global__ void __launch_bounds__(DE_CURVE_THREADS)
    de_curves_kernel(DeArgs a, const float* __restrict__ score, const int32_t* __restrict__ gt_cls, const int32_t* __restrict__ cls_off,
                     const uint32_t* __restrict__ ord, const int32_t* __restrict__ match_s, const double* __restrict__ errs,
                     uint32_t* __restrict__ tpcum, double* __restrict__ mconf, double* __restrict__ cm, double* __restrict__ curves,
                     double* __restrict__ stats) {
  __shared__ DeAcc wave_tot[DE_CURVE_THREADS / 64];
  __shared__ uint32_t npos_w[DE_CURVE_THREADS / 64];
  const int c = blockIdx.x / a.T, t = blockIdx.x % a.T;
  const int64_t lo = de_clamp(cls_off[c], 0, a.P), n = de_clamp(cls_off[c + 1], lo, a.P) - lo;
  uint32_t mine = 0;
  for (int64_t g = threadIdx.x; g < a.G; g += DE_CURVE_THREADS) mine += gt_cls[g] == c ? 1u : 0u;
  mine = fsf_wave_sum(mine);
  if (fsf_lane() == 0) npos_w[threadIdx.x >> 6] = mine;
  __syncthreads();
  uint32_t npos = 0;
  for (int w = 0; w < DE_CURVE_THREADS / 64; ++w) npos += npos_w[w];
  DeAcc carry;
  carry.tp = 0;
  for (int e = 0; e < DE_ERRS; ++e) {
    carry.cnt[e] = 0;
    carry.sum[e] = 0.0;
  }
  const bool with_err = t == a.t_tp;
  if (with_err)
    de_curve_tiles<true>(a, t, lo, n, match_s, errs, score, ord, tpcum, mconf, cm, carry, wave_tot);
  else
    de_curve_tiles<false>(a, t, lo, n, match_s, errs, score, ord, tpcum, mconf, cm, carry, wave_tot);
  __threadfence();
  __syncthreads();  // tpcum / mconf / cm of this class are read back below by other threads of the workgroup
  const int64_t ntp = carry.tp;
  const bool none = npos == 0 || n == 0 || ntp == 0;  // the specification's no_predictions
  double* st = stats + (int64_t)blockIdx.x * 8;
  if (threadIdx.x == 0) {
    int nan_bits = 0;
    for (int e = 0; e < DE_ERRS; ++e) nan_bits |= (carry.cnt[e] == 0 ? 1 : 0) << e;
    st[0] = (double)ntp; st[1] = none ? 1.0 : 0.0; st[2] = (double)npos; st[3] = (double)n; st[4] = (double)nan_bits;
    st[5] = st[6] = st[7] = 0.0;
  }
  const int i = threadIdx.x;
  if (i >= DE_PTS) return;
  const int rows = 2 * a.T + DE_ERRS;
  double* prec_out = curves + ((int64_t)c * rows + t) * DE_PTS;
  double* conf_out = curves + ((int64_t)c * rows + a.T + t) * DE_PTS;
  double* err_out = curves + ((int64_t)c * rows + 2 * a.T) * DE_PTS;
  if (none) {
    prec_out[i] = 0.0;
    conf_out[i] = 0.0;
    if (with_err)
      for (int e = 0; e < DE_ERRS; ++e) err_out[e * DE_PTS + i] = 1.0;
    return;
  }
  const double x = i == DE_PTS - 1 ? 1.0 : __dmul_rn((double)i, 1.0 / (DE_PTS - 1));  // np.linspace(0, 1, 101)[i]
  const DeCurveView v{tpcum + (int64_t)t * a.P, ord, score, lo + n, (double)npos};
  double pi, ci;
  if (x > v.rec(n - 1)) {
    pi = ci = 0.0;  // right = 0
  } else if (x < v.rec(0)) {
    pi = v.prec(0);
    ci = v.conf(0);
  } else {
    int64_t j = 0, up = n - 1;  // the largest j with rec(j) <= x
    while (j < up) {
      const int64_t mid = j + (up - j + 1) / 2;
      if (v.rec(mid) <= x) j = mid; else up = mid - 1;
    }
    const double xj = v.rec(j);
    if (j == n - 1 || xj == x) {
      pi = v.prec(j);
      ci = v.conf(j);
    } else {
      const double dx = v.rec(j + 1) - xj;
      pi = (v.prec(j + 1) - v.prec(j)) / dx * (x - xj) + v.prec(j);
      ci = (v.conf(j + 1) - v.conf(j)) / dx * (x - xj) + v.conf(j);
    }
  }
  prec_out[i] = pi;
  conf_out[i] = ci;
  if (!with_err) return;
  // np.interp(conf_interp[::-1], match_conf[::-1], cummean[::-1])[::-1]: match_conf falls along m, so the largest reversed index with
  // xp <= x is the SMALLEST m with mconf[m] <= x
  const double* mc = mconf + lo;
  for (int e = 0; e < DE_ERRS; ++e) {
    const double* f = cm + e * a.P + lo;
    double r;
    if (carry.cnt[e] == 0) {
      r = 1.0;  // cummean of an all-NaN input is ones
    } else if (ci > mc[0]) {
      r = f[0];
    } else if (ci < mc[ntp - 1]) {
      r = f[ntp - 1];
    } else {
      int64_t m = 0, up = ntp - 1;
      while (m < up) {
        const int64_t mid = m + (up - m) / 2;
        if (mc[mid] <= ci) up = mid; else m = mid + 1;
      }
      if (m == 0 || mc[m] == ci)
        r = f[m];
      else
        r = (f[m - 1] - f[m]) / (mc[m - 1] - mc[m]) * (ci - mc[m]) + f[m];
    }
    err_out[e * DE_PTS + i] = r;
  }
}

// K41c: result f64 [8 + C (2 T + 7) ... ] — see FSF_DET_EVAL_* in the header
__global__ void __launch_bounds__(256)
    de_summary_kernel(DeArgs a, const double* __restrict__ curves, const double* __restrict__ stats,
                      double* __restrict__ result) {
  const int C = a.C, T = a.T, rows = 2 * T + DE_ERRS;
  double* ap = result + FSF_DET_EVAL_HEAD;
  double* tpe = ap + C * T;
  double* npos = tpe + C * DE_ERRS;
  double* npred = npos + C;
  double* ntp = npred + C;
  double* none = ntp + C * T;
  for (int k = threadIdx.x; k < C * T; k += blockDim.x) {
    const int c = k / T, t = k % T;
    const double* prec = curves + ((int64_t)c * rows + t) * DE_PTS;
    double s = 0.0;
    for (int i = a.first; i < DE_PTS; ++i) {
      const double v = prec[i] - a.min_precision;
      s += v < 0.0 ? 0.0 : v;
    }
    ap[k] = a.first < DE_PTS ? s / (double)(DE_PTS - a.first) / (1.0 - a.min_precision) : __builtin_nan("");
    ntp[k] = stats[k * 8 + 0];
    none[k] = stats[k * 8 + 1];
    if (t == a.t_tp) {
      npos[c] = stats[k * 8 + 2];
      npred[c] = stats[k * 8 + 3];
    }
  }
  for (int k = threadIdx.x; k < C * DE_ERRS; k += blockDim.x) {
    const int c = k / DE_ERRS, e = k % DE_ERRS;
    const double* conf = curves + ((int64_t)c * rows + T + a.t_tp) * DE_PTS;
    const double* err = curves + ((int64_t)c * rows + 2 * T + e) * DE_PTS;
    int last = 0;
    for (int i = 0; i < DE_PTS; ++i)
      if (conf[i] != 0.0) last = i;
    double r = 1.0;
    if (last >= a.first) {
      double s = 0.0;
      for (int i = a.first; i <= last; ++i) s += err[i];
      r = s / (double)(last - a.first + 1);
    }
    tpe[k] = ((a.flags[c] >> (1 + e)) & 1) ? __builtin_nan("") : r;  // the class does not define this error
  }
  __threadfence();
  __syncthreads();
  if (threadIdx.x != 0) return;
  double s = 0.0;
  for (int k = 0; k < C * T; ++k) s += ap[k];
  const double map = s / (double)(C * T);
  double score_sum = 0.0;
  for (int e = 0; e < DE_ERRS; ++e) {
    double es = 0.0;
    int cnt = 0;
    for (int c = 0; c < C; ++c) {
      const double v = tpe[c * DE_ERRS + e];
      if (v == v) {
        es += v;
        ++cnt;
      }
    }
    const double m = cnt ? es / (double)cnt : __builtin_nan("");  // np.nanmean
    result[1 + e] = m;
    const double sc = 1.0 - m;
    score_sum += sc == sc ? (sc > 0.0 ? sc : 0.0) : sc;  // Python's max(1 - err, 0.0) keeps a NaN
  }
  result[0] = map;
  result[6] = (a.ap_weight * map + score_sum) / (a.ap_weight + (double)DE_ERRS);
  result[7] = 0.0;
}

static bool de_sizes_ok(int64_t P, int64_t G, int64_t S, int64_t C, int64_t T) {
  return P >= 0 && G >= 0 && S >= 0 && C >= 1 && C <= FSF_DET_EVAL_MAX_CLASSES && T >= 1 && T <= FSF_DET_EVAL_MAX_THRESHOLDS;
}
// every count the u32 scan words, the i32 offsets and the sort's values carry stays below 2^30
static bool de_sizes_supported(int64_t P, int64_t G, int64_t S, int64_t C, int64_t T) {
  const int64_t lim = (int64_t)1 << 30;
  return P * T < lim && G * T < lim && S * (C + 1) < lim;
}

}  // namespace fsf

using namespace fsf;

extern "C" int64_t fsf_det_eval_scratch_bytes(int64_t num_pred, int64_t num_gt, int64_t num_samples, int32_t num_classes,
                                                int32_t num_thresholds) {
  if (!de_sizes_ok(num_pred, num_gt, num_samples, num_classes, num_thresholds) ||
      !de_sizes_supported(num_pred, num_gt, num_samples, num_classes, num_thresholds))
    return 0;
  return fsf_layout_bytes<DetEvalLayout>(num_pred, num_gt, num_samples, (int64_t)num_classes, (int64_t)num_thresholds);
}

extern "C" int64_t fsf_det_eval_result_words(int32_t num_classes, int32_t num_thresholds) {
  return FSF_DET_EVAL_HEAD + (int64_t)num_classes * (3 * (int64_t)num_thresholds + DE_ERRS + 2);
}

extern "C" int fsf_det_eval_compute(const float* pred, const float* score, const int32_t* pred_label, const int32_t* pred_attr,
                                    const int32_t* pred_sample, int64_t num_pred, const float* gt, const int32_t* gt_label,
                                    const int32_t* gt_attr, const int32_t* gt_sample, int64_t num_gt, int64_t num_samples,
                                    int32_t num_classes, const int32_t* class_flags, const double* class_range, const double* dist_ths,
                                    int32_t num_thresholds, int32_t tp_threshold, int32_t first_recall, const double* params, int32_t* match,
                                    double* curves, double* result, void* workspace, int64_t workspace_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const int64_t P = num_pred, G = num_gt, S = num_samples;
  const int C = num_classes, T = num_thresholds;
  if (!de_sizes_ok(P, G, S, C, T) || !class_flags || !dist_ths || !params || !curves || !result || tp_threshold < 0 || tp_threshold >= T ||
      first_recall < 0 || first_recall > DE_PTS)
    return FSF_ERR_INVALID_ARG;
  if ((P > 0 && (!pred || !score || !pred_label || !pred_attr || !pred_sample || !match)) || (G > 0 && (!gt || !gt_label || !gt_attr || !gt_sample)) ||
      ((P > 0 || G > 0) && S < 1))
    return FSF_ERR_INVALID_ARG;
  if (!de_sizes_supported(P, G, S, C, T)) return FSF_ERR_UNSUPPORTED;
  if (!(params[0] >= 0.0 && params[0] < 1.0)) return FSF_ERR_INVALID_ARG;  // min_precision
  FSF_CARVE(DetEvalLayout, L, workspace, workspace_bytes, P, G, S, (int64_t)C, (int64_t)T);
  DeArgs a;
  a.P = P; a.G = G; a.S = (int)S; a.C = C; a.T = T; a.t_tp = tp_threshold; a.first = first_recall;
  a.min_precision = params[0];
  a.ap_weight = params[1];
  for (int t = 0; t < FSF_DET_EVAL_MAX_THRESHOLDS; ++t) a.ths[t] = t < T ? dist_ths[t] : 0.0;

  a.use_range = class_range ? 1 : 0;
  for (int c = 0; c < FSF_DET_EVAL_MAX_CLASSES; ++c) {
    a.flags[c] = c < C ? class_flags[c] : 0;
    a.range[c] = (class_range && c < C) ? class_range[c] : 0.0;
  }
  FSF_HIP_TRY(hipMemsetAsync(L.taken, 0, (size_t)(T * G > 0 ? T * G : 1), stream));
  const int64_t most = P > G ? P : G;
  hipLaunchKernelGGL(de_prep_kernel, dim3(fsf_stream_grid(most + 1, 256)), dim3(256), 0, stream, a, pred, score, pred_label, gt, gt_label,
                     gt_sample, L.sort.keys_a, L.sort.vals_a, match, L.gt_cls, L.gt_off);
  FSF_LAUNCH_CHECK();
  uint64_t* keys_sorted = L.sort.keys_a;
  uint32_t* vals_sorted = L.sort.vals_a;
  if (P > 0) {
    int class_bits = 1;
    while ((1 << class_bits) <= C) ++class_bits;
    const int rc = radix_sort_pairs(L.sort.keys_a, L.sort.vals_a, L.sort.keys_b, L.sort.vals_b, L.sort.hist, P, 32 + class_bits, &keys_sorted,
                                    &vals_sorted, stream);
    if (rc != FSF_OK) return rc;
  }
  // sort B reads its input from the pair sort A did not end in, and may clobber sort A's result: `ord` and `cls_off` keep what is needed
  uint64_t* keys2 = keys_sorted == L.sort.keys_a ? L.sort.keys_b : L.sort.keys_a;
  uint32_t* vals2 = vals_sorted == L.sort.vals_a ? L.sort.vals_b : L.sort.vals_a;
  hipLaunchKernelGGL(de_order_kernel, dim3(fsf_stream_grid(P + 1, 256)), dim3(256), 0, stream, a, keys_sorted, vals_sorted, pred_sample, keys2,
                     vals2, L.ord, L.cls_off);
  FSF_LAUNCH_CHECK();
  uint64_t* keys2_sorted = keys2;
  uint32_t* seg_order = vals2;
  if (P > 0) {
    int seg_bits = 1;
    while (((int64_t)1 << seg_bits) < S * (C + 1)) ++seg_bits;
    const int rc = radix_sort_pairs(keys2, vals2, keys_sorted, vals_sorted, L.sort.hist, P, seg_bits, &keys2_sorted, &seg_order, stream);
    if (rc != FSF_OK) return rc;
  }
  hipLaunchKernelGGL(de_seg_bounds_kernel, dim3(fsf_stream_grid(P + 1, 256)), dim3(256), 0, stream, a, keys2_sorted, L.seg_off);
  FSF_LAUNCH_CHECK();
  if (P > 0) {
    const int64_t items = S * C * T;
    const int64_t blocks = (items + 3) / 4;  // most segments are empty and leave at once: the grid strides beyond 16384 workgroups
    hipLaunchKernelGGL(de_match_kernel, dim3((unsigned)(blocks < 16384 ? blocks : 16384)), dim3(256), 0, stream,
                       a, pred, pred_attr, gt, gt_attr, L.gt_cls, L.gt_off, L.seg_off, seg_order, L.ord, L.taken, match,
                       L.match_s, L.errs);
    FSF_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(de_curves_kernel, dim3(C * T), dim3(DE_CURVE_THREADS), 0, stream, a, score, L.gt_cls, L.cls_off, L.ord, L.match_s,
                     L.errs, L.tpcum, L.mconf, L.cm, curves, L.stats);
  FSF_LAUNCH_CHECK();
  hipLaunchKernelGGL(de_summary_kernel, dim3(1), dim3(256), 0, stream, a, curves, L.stats, result);
  FSF_LAUNCH_CHECK();
  return FSF_OK;
}
