// K39  optimizer step on the gradient buckets (include/fsf_hip.h, docs/kernels/K39_optimizer_step.md): the global gradient norm as
// float64 partials (K39a), then clip coefficient + AdamW + gradient clear in one streaming pass (K39b).
//
// Both kernels walk the caller's chunk table: one row = up to FSF_OPTIM_CHUNK elements of ONE parameter, with the addresses of the
// parameter, its gradient inside a bucket and its two moments.  A workgroup takes rows w, w + W, ...; thread t of a row takes the
// elements 4 (t + 256 k) .. + 3.  That assignment is the same whether an address allows 16-byte accesses or not, and the arithmetic
// per element is the same scalar code, so the aligned and the unaligned form of a row give the same bits (and K39a the same sum).
//
// The arithmetic of K39b, pinned (every line one IEEE f32 operation per operator, -ffp-contract=off: no fma; sqrt and / are the
// correctly rounded ones, hipcc's default for HIP):
//     g = g_raw * coef                                       coef = 1 without clipping
//     p = p * decay_factor[G]
//     m = w < 0.5 ? m + w * (g - m) : g - (g - m) * (1 - w)   w = one_minus_beta1 (torch's lerp)
//     v = v * beta2 + (one_minus_beta2 * g) * g
//     denom = sqrt(v) / bc2_sqrt + eps
//     p = p - step_size[G] * (m / denom)
// fullysparsefusion_amd/optim.py (`FusedAdamW(fused=False)`) states the same in torch operations; tests/test_optim_gpu.py holds the two
// to the same bits.
#include "common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kStride = kBlock * 4;  // elements a workgroup takes per round
static_assert(FSF_OPTIM_CHUNK % kStride == 0, "a full chunk is a whole number of rounds");
static_assert((FSF_OPTIM_MAX_GROUPS & (FSF_OPTIM_MAX_GROUPS - 1)) == 0, "the group id is masked");

struct Chunk {
  float* p;
  float* g;
  float* m;
  float* v;
  int32_t count;
  int32_t group;
};
static_assert(sizeof(Chunk) == 8 * FSF_OPTIM_TABLE_WORDS, "one table row");

struct StepScalars {
  float decay[FSF_OPTIM_MAX_GROUPS];
  float step[FSF_OPTIM_MAX_GROUPS];
  float w, beta2, omb2, bc2_sqrt, eps, max_norm;
};

__device__ __forceinline__ bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// x[0 .. valid) <- q[0 .. valid): one 16-byte load where the address allows it and all four are there, else one float at a time
__device__ __forceinline__ void load4(const float* q, bool vec, int valid, float (&x)[4]) {
  if (vec && valid == 4) {
    const float4 t = *reinterpret_cast<const float4*>(q);
    x[0] = t.x, x[1] = t.y, x[2] = t.z, x[3] = t.w;
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) x[i] = i < valid ? q[i] : 0.0f;
  }
}

__device__ __forceinline__ void store4(float* q, bool vec, int valid, const float (&x)[4]) {
  if (vec && valid == 4) {
    *reinterpret_cast<float4*>(q) = make_float4(x[0], x[1], x[2], x[3]);
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (i < valid) q[i] = x[i];
  }
}

// the 256 thread values added as a fixed tree; every thread gets the total
__device__ __forceinline__ double block_sum(double a, double* lds) {
  const int t = threadIdx.x;
  lds[t] = a;
  __syncthreads();
#pragma unroll
  for (int o = kBlock / 2; o > 0; o >>= 1) {
    if (t < o) lds[t] += lds[t + o];
    __syncthreads();
  }
  const double total = lds[0];
  __syncthreads();
  return total;
}

// K39a
__global__ __launch_bounds__(kBlock) void optim_grad_sumsq_kernel(const Chunk* __restrict__ table, int64_t num_chunks,
                                                                   double* __restrict__ partials) {
  __shared__ double lds[kBlock];
  double acc = 0.0;
  for (int64_t c = blockIdx.x; c < num_chunks; c += gridDim.x) {
    const Chunk ch = table[c];
    const int count = ch.count < FSF_OPTIM_CHUNK ? ch.count : FSF_OPTIM_CHUNK;
    const bool vec = aligned16(ch.g);
    for (int base = threadIdx.x * 4; base < count; base += kStride) {
      const int valid = count - base < 4 ? count - base : 4;
      float g[4];
      load4(ch.g + base, vec, valid, g);
#pragma unroll
      for (int i = 0; i < 4; ++i) acc += (double)g[i] * (double)g[i];  // (elements past the end were loaded as 0)
    }
  }
  const double total = block_sum(acc, lds);
  if (threadIdx.x == 0) partials[blockIdx.x] = total;
}

// K39b
__global__ __launch_bounds__(kBlock) void optim_adamw_step_kernel(const Chunk* __restrict__ table, int64_t num_chunks, StepScalars s,
                                                                   const double* __restrict__ partials, int num_partials, int zero_grads,
                                                                   float* __restrict__ grad_norm) {
  __shared__ double lds[kBlock];
  float coef = 1.0f;
  if (num_partials > 0) {  // (clipping; uniform over the grid)
    double a = 0.0;
    for (int i = threadIdx.x; i < num_partials; i += kBlock) a += partials[i];
    const float norm = (float)sqrt(block_sum(a, lds));
    const float c = s.max_norm / (norm + 1e-6f);
    coef = c > 1.0f ? 1.0f : c;  // (a NaN stays)
    if (blockIdx.x == 0 && threadIdx.x == 0) grad_norm[0] = norm;
  }
  const float w = s.w, one_minus_w = 1.0f - s.w;
  const bool small_w = w < 0.5f;
  for (int64_t c = blockIdx.x; c < num_chunks; c += gridDim.x) {
    const Chunk ch = table[c];
    const int count = ch.count < FSF_OPTIM_CHUNK ? ch.count : FSF_OPTIM_CHUNK;
    const float decay = s.decay[ch.group & (FSF_OPTIM_MAX_GROUPS - 1)], step = s.step[ch.group & (FSF_OPTIM_MAX_GROUPS - 1)];
    const bool vp = aligned16(ch.p), vg = aligned16(ch.g), vm = aligned16(ch.m), vv = aligned16(ch.v);
    for (int base = threadIdx.x * 4; base < count; base += kStride) {
      const int valid = count - base < 4 ? count - base : 4;
      float p[4], g[4], m[4], v[4];
      load4(ch.p + base, vp, valid, p);
      load4(ch.g + base, vg, valid, g);
      load4(ch.m + base, vm, valid, m);
      load4(ch.v + base, vv, valid, v);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float gi = g[i] * coef;
        float pi = p[i] * decay;
        const float d = gi - m[i];
        const float mi = small_w ? m[i] + w * d : gi - d * one_minus_w;
        const float vi = v[i] * s.beta2 + (s.omb2 * gi) * gi;
        const float denom = sqrtf(vi) / s.bc2_sqrt + s.eps;
        pi = pi - step * (mi / denom);
        p[i] = pi, m[i] = mi, v[i] = vi, g[i] = 0.0f;
      }
      store4(ch.p + base, vp, valid, p);
      store4(ch.m + base, vm, valid, m);
      store4(ch.v + base, vv, valid, v);
      if (zero_grads) store4(ch.g + base, vg, valid, g);
    }
  }
}

int num_partials_of(int64_t num_chunks) {
  return (int)(num_chunks < FSF_OPTIM_MAX_PARTIALS ? (num_chunks < 1 ? 1 : num_chunks) : FSF_OPTIM_MAX_PARTIALS);
}

}  // namespace

extern "C" int64_t fsf_optim_table_bytes(int64_t num_chunks) {
  return (int64_t)sizeof(Chunk) * (num_chunks > 0 ? num_chunks : 0);
}

extern "C" int64_t fsf_optim_workspace_bytes(int64_t num_chunks) { return (int64_t)sizeof(double) * num_partials_of(num_chunks); }

extern "C" int fsf_optim_grad_sumsq(const int64_t* table, int64_t num_chunks, void* workspace, int64_t workspace_bytes, void* stream) {
  if (num_chunks < 0) return FSF_ERR_INVALID_ARG;
  if (num_chunks == 0) return FSF_OK;
  if (table == nullptr || workspace == nullptr) return FSF_ERR_INVALID_ARG;
  if (workspace_bytes < fsf_optim_workspace_bytes(num_chunks)) return FSF_ERR_WORKSPACE;
  optim_grad_sumsq_kernel<<<num_partials_of(num_chunks), kBlock, 0, (hipStream_t)stream>>>((const Chunk*)table, num_chunks,
                                                                                           (double*)workspace);
  FSF_LAUNCH_CHECK();
  return FSF_OK;
}

extern "C" int fsf_optim_adamw_step(const int64_t* table, int64_t num_chunks, int32_t num_groups,
                                    const float decay_factor[FSF_OPTIM_MAX_GROUPS], const float step_size[FSF_OPTIM_MAX_GROUPS],
                                    float one_minus_beta1, float beta2, float one_minus_beta2, float bc2_sqrt, float eps, float max_norm,
                                    int32_t clip, int32_t zero_grads, const void* workspace, int64_t workspace_bytes, float* grad_norm,
                                    void* stream) {
  if (num_chunks < 0) return FSF_ERR_INVALID_ARG;
  if (num_chunks == 0) return FSF_OK;
  if (num_groups > FSF_OPTIM_MAX_GROUPS) return FSF_ERR_UNSUPPORTED;
  if (table == nullptr || num_groups < 1 || decay_factor == nullptr || step_size == nullptr) return FSF_ERR_INVALID_ARG;
  if (clip) {
    if (workspace == nullptr || grad_norm == nullptr) return FSF_ERR_INVALID_ARG;
    if (workspace_bytes < fsf_optim_workspace_bytes(num_chunks)) return FSF_ERR_WORKSPACE;
  }
  StepScalars s;
  for (int i = 0; i < FSF_OPTIM_MAX_GROUPS; ++i) {
    s.decay[i] = i < num_groups ? decay_factor[i] : 1.0f;
    s.step[i] = i < num_groups ? step_size[i] : 0.0f;
  }
  s.w = one_minus_beta1, s.beta2 = beta2, s.omb2 = one_minus_beta2, s.bc2_sqrt = bc2_sqrt, s.eps = eps, s.max_norm = max_norm;
  const int grid = (int)(num_chunks < 2048 ? num_chunks : 2048);  // 256 CUs x 8 workgroups, the rest by stride
  optim_adamw_step_kernel<<<grid, kBlock, 0, (hipStream_t)stream>>>((const Chunk*)table, num_chunks, s, (const double*)workspace,
                                                                    clip ? num_partials_of(num_chunks) : 0, zero_grads, grad_norm);
  FSF_LAUNCH_CHECK();
  return FSF_OK;
}
