// The weight side of the f16 hi | lo operand format: max |w| of a layer into its planes' header.  See operand_formats.h.
#include <algorithm>

#include "operand_formats.h"

namespace fsf {

// max |w| over the layer -> hdr[FMT_HDR_AMAX_BITS] (bit pattern; cleared by the caller), one atomic per workgroup
__global__ void __launch_bounds__(256) fmt_weight_absmax_kernel(const float* __restrict__ w, int64_t n, unsigned* __restrict__ hdr) {
  __shared__ float wave_max[4];
  float amax = 0.0f;
  // 16-byte loads over the aligned body; the (at most 3 + 3) scalars in front of / behind it go to workgroup 0
  const int64_t head = std::min<int64_t>(n, (int64_t)(((16 - (reinterpret_cast<uintptr_t>(w) & 15)) & 15) >> 2));
  const int64_t n4 = (n - head) >> 2;
  const float4* w4 = reinterpret_cast<const float4*>(w + head);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    const float4 v = w4[i];
    amax = fmaxf(fmaxf(amax, fabsf(v.x)), fmaxf(fabsf(v.y), fmaxf(fabsf(v.z), fabsf(v.w))));
  }
  if (blockIdx.x == 0) {
    if ((int64_t)threadIdx.x < head) amax = fmaxf(amax, fabsf(w[threadIdx.x]));
    const int64_t tail0 = head + (n4 << 2);
    if (tail0 + threadIdx.x < n && threadIdx.x < 4) amax = fmaxf(amax, fabsf(w[tail0 + threadIdx.x]));
  }
  amax = fsf_wave_max(amax);
  if ((threadIdx.x & 63) == 0) wave_max[threadIdx.x >> 6] = amax;
  __syncthreads();
  // one atomic per workgroup (per-wave atomics on the one address were the whole cost of this kernel: 84 us for 1.8 MB);
  // |x| bit patterns order like the values
  if (threadIdx.x == 0)
    atomicMax(hdr + FMT_HDR_AMAX_BITS, __float_as_uint(fmaxf(fmaxf(wave_max[0], wave_max[1]), fmaxf(wave_max[2], wave_max[3]))));
}

int fsf_weight_layer_absmax(const float* w, int64_t n, void* hdr, hipStream_t stream) {
  FSF_HIP_TRY(hipMemsetAsync(hdr, 0, FMT_HDR_BYTES, stream));
  // (at most 256 workgroups: each ends in ONE atomic on the same word — 2 048 of them took 25 us for a 1 M-element weight)
  hipLaunchKernelGGL(fmt_weight_absmax_kernel, dim3((unsigned)std::min<int64_t>(256, (n / 4 + 255) / 256 + 1)), dim3(256), 0, stream, w, n,
                     (unsigned*)hdr);
  FSF_LAUNCH_CHECK();
  return FSF_OK;
}

}  // namespace fsf
