// K13c: backward of the bilinear image-feature gather (K13b, project.hip) with respect to the feature map — see include/fsf_hip.h and
// docs/kernels/K13c_bilinear_backward.md.  The exact transpose of the forward, grad_feat[cam, :, y, x] = sum of a_k(i, cam) * grad_out
// row over every tap that lands on the texel, as a GATHER: no float atomics, the summation order is a function of the input alone.
//   K13c-a  one lane per entry e = i * ncam + cam: the forward's taps (bilinear_taps.h, the same bits) -> the pair (top-left cell id, e)
//           and the fractions (wx1, wy1).  Cells are the (Hf + 1) x (Wf + 1) positions a top-left corner can take, x0 in [-1, Wf - 1],
//           y0 in [-1, Hf - 1]; an invalid projection gets the sentinel NC = ncam (Hf + 1)(Wf + 1) and sorts behind every cell.
//   sort    the stable radix sort of the n * ncam pairs on ceil(log2(NC + 1)) key bits: ties keep source order.
//   starts  start[c] = lower_bound(sorted keys, c), c in [0, NC], one lane per cell.
//   K13c-b  one wave per texel (cam, y, x): its four 16-lane teams take the four cells (y - dy, x - dx) that reach it, each walks its
//           cell's run in sorted order and accumulates a * grad_out[row] per channel in fp32 (a run longer than FSF_BILINEAR_BWD_CHUNK in
//           chunks, the chunk partials added in chunk order); the four team sums are added in the order (dy, dx) = 00, 01, 10, 11 and
//           the texel is stored — every texel, so grad_feat needs no clearing.
#include "bilinear_taps.h"
#include "common.h"
#include "radix_sort.h"

namespace fsf {

struct BilinBwdKeyArgs {
  const float* xyz;
  const float* lidar2img;
  uint64_t* keys;
  uint32_t* vals;
  float2* frac;
  int64_t total;  // n * ncam
  int stride, ncam, Hf, Wf, img_h, img_w;
};

// K13c-a
__global__ void __launch_bounds__(256) bilinear_bwd_keys_kernel(BilinBwdKeyArgs a) {
  extern __shared__ float s_mat[];
  for (int t = threadIdx.x; t < a.ncam * 12; t += blockDim.x) s_mat[t] = a.lidar2img[(t / 12) * 16 + t % 12];
  __syncthreads();
  const float fw = (float)a.img_w, fh = (float)a.img_h;
  const int64_t cells_cam = (int64_t)(a.Hf + 1) * (a.Wf + 1);
  const uint64_t sentinel = (uint64_t)(a.ncam * cells_cam);
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < a.total; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = e / a.ncam;
    const int cam = (int)(e - i * a.ncam);
    const float* p = a.xyz + i * a.stride;
    const BilinearTaps tp = bilinear_taps(s_mat + cam * 12, p[0], p[1], p[2], fw, fh, a.Hf, a.Wf);
    // (a valid projection cannot leave the cell grid; the test keeps a key above NC, which the sort's key bits do not cover, impossible)
    const bool in_cells = tp.valid && tp.x0 >= -1 && tp.x0 < a.Wf && tp.y0 >= -1 && tp.y0 < a.Hf;
    a.keys[e] = in_cells ? (uint64_t)(cam * cells_cam + (int64_t)(tp.y0 + 1) * (a.Wf + 1) + (tp.x0 + 1)) : sentinel;
    a.vals[e] = (uint32_t)e;
    a.frac[e] = make_float2(tp.wx1, tp.wy1);
  }
}

// start[c] = the first sorted position whose key is >= c, c in [0, num_cells] (start[num_cells] = the number of valid entries)
__global__ void __launch_bounds__(256)
    bilinear_bwd_starts_kernel(const uint64_t* __restrict__ keys, int64_t total, int64_t num_cells, uint32_t* __restrict__ start) {
  for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c <= num_cells; c += (int64_t)gridDim.x * blockDim.x) {
    int64_t lo = 0, hi = total;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (keys[mid] < (uint64_t)c) lo = mid + 1; else hi = mid;
    }
    start[c] = (uint32_t)lo;
  }
}

struct BilinBwdSumArgs {
  const uint32_t* vals;   // sorted entries
  const uint32_t* start;  // [NC + 1]
  const float2* frac;     // [n * ncam], by entry
  const float* grad_out;
  float* grad_feat;
  int64_t texels;  // ncam * Hf * Wf
  int ncam, C, Hf, Wf, channels_last, reduce;
};

template <int W>
struct BwdVec;
template <>
struct BwdVec<4> {
  float4 v;
  __device__ __forceinline__ void zero() { v = make_float4(0.f, 0.f, 0.f, 0.f); }
  __device__ __forceinline__ void load(const float* p) { v = *reinterpret_cast<const float4*>(p); }
  __device__ __forceinline__ void add_scaled(float a, const BwdVec& g) {
    v.x += a * g.v.x; v.y += a * g.v.y; v.z += a * g.v.z; v.w += a * g.v.w;
  }
  __device__ __forceinline__ void add(const BwdVec& o) { v.x += o.v.x; v.y += o.v.y; v.z += o.v.z; v.w += o.v.w; }
  __device__ __forceinline__ BwdVec from_lane(int lane) const {
    BwdVec r;
    r.v = make_float4(__shfl(v.x, lane), __shfl(v.y, lane), __shfl(v.z, lane), __shfl(v.w, lane));
    return r;
  }
  __device__ __forceinline__ float at(int j) const { return j == 0 ? v.x : j == 1 ? v.y : j == 2 ? v.z : v.w; }
};
template <>
struct BwdVec<1> {
  float v;
  __device__ __forceinline__ void zero() { v = 0.f; }
  __device__ __forceinline__ void load(const float* p) { v = *p; }
  __device__ __forceinline__ void add_scaled(float a, const BwdVec& g) { v += a * g.v; }
  __device__ __forceinline__ void add(const BwdVec& o) { v += o.v; }
  __device__ __forceinline__ BwdVec from_lane(int lane) const {
    BwdVec r;
    r.v = __shfl(v, lane);
    return r;
  }
  __device__ __forceinline__ float at(int) const { return v; }
};

// K13c-b.  W = 4: C % 4 == 0 and grad_out (and a channels-last grad_feat) 16-byte aligned: a lane owns four channels.
template <int W>
__global__ void __launch_bounds__(256) bilinear_bwd_sum_kernel(BilinBwdSumArgs a) {
  using V = BwdVec<W>;
  const int lane = threadIdx.x & 63, tl = lane & 15, q = lane >> 4;
  const int dy = q >> 1, dx = q & 1;
  const int64_t plane = (int64_t)a.Hf * a.Wf;
  const int64_t cells_cam = (int64_t)(a.Hf + 1) * (a.Wf + 1);
  const int64_t waves = (int64_t)gridDim.x * 4;
  for (int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); t < a.texels; t += waves) {
    const int cam = (int)(t / plane);
    const int64_t pix = t - (int64_t)cam * plane;
    const int y = (int)(pix / a.Wf), x = (int)(pix - (int64_t)y * a.Wf);
    // the team's cell: top-left corner (y - dy, x - dx), rows / columns shifted by one (always inside the cell grid)
    const int64_t cell = cam * cells_cam + (int64_t)(y - dy + 1) * (a.Wf + 1) + (x - dx + 1);
    const int64_t lo = a.start[cell], hi = a.start[cell + 1];
    for (int cb = 0; cb < a.C; cb += 16 * W) {  // (uniform over the wave: the team sums meet in shuffles below)
      const int c = cb + tl * W;
      V acc;
      acc.zero();
      if (c < a.C) {
        for (int64_t cs = lo; cs < hi; cs += FSF_BILINEAR_BWD_CHUNK) {
          const int64_t ce = cs + FSF_BILINEAR_BWD_CHUNK < hi ? cs + FSF_BILINEAR_BWD_CHUNK : hi;
          V part;
          part.zero();
          int64_t s = cs;
          for (; s + 4 <= ce; s += 4) {  // four rows in flight; added in sorted order
            float w[4];
            V g[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const uint32_t e = a.vals[s + j];
              const float2 f = a.frac[e];
              w[j] = (dx ? f.x : 1.0f - f.x) * (dy ? f.y : 1.0f - f.y);
              const int64_t row = a.reduce ? (int64_t)(e / (uint32_t)a.ncam) : (int64_t)e;
              g[j].load(a.grad_out + row * a.C + c);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) part.add_scaled(w[j], g[j]);
          }
          for (; s < ce; ++s) {
            const uint32_t e = a.vals[s];
            const float2 f = a.frac[e];
            const float w = (dx ? f.x : 1.0f - f.x) * (dy ? f.y : 1.0f - f.y);
            const int64_t row = a.reduce ? (int64_t)(e / (uint32_t)a.ncam) : (int64_t)e;
            V g;
            g.load(a.grad_out + row * a.C + c);
            part.add_scaled(w, g);
          }
          acc.add(part);
        }
      }
      V tot = acc.from_lane(tl);
      tot.add(acc.from_lane(tl + 16));
      tot.add(acc.from_lane(tl + 32));
      tot.add(acc.from_lane(tl + 48));
      if (q == 0 && c < a.C) {
        if (a.channels_last) {
          float* o = a.grad_feat + t * a.C + c;
          if (W == 4) {
            *reinterpret_cast<float4*>(o) = make_float4(tot.at(0), tot.at(1), tot.at(2), tot.at(3));
          } else {
            o[0] = tot.at(0);
          }
        } else {
          float* o = a.grad_feat + ((int64_t)cam * a.C + c) * plane + pix;
#pragma unroll
          for (int j = 0; j < W; ++j) o[(int64_t)j * plane] = tot.at(j);
        }
      }
    }
  }
}

struct BilinBwdLayout {
  RadixScratch sort;
  float2* frac;
  uint32_t* start;
  BilinBwdLayout(FsfArena& ar, int64_t total, int64_t num_cells)
      : sort(ar, total), frac(ar.take<float2>(total)), start(ar.take<uint32_t>(num_cells + 1)) {}
};

// 0: fine; otherwise the status the arguments earn (shared by the size function, which answers 0 bytes to them)
static int bilinear_bwd_shape_status(int64_t n, int32_t ncam, int32_t feat_h, int32_t feat_w, int32_t channels) {
  if (n < 0 || ncam < 1 || ncam > 64 || channels < 1 || feat_h < 1 || feat_w < 1) return FSF_ERR_INVALID_ARG;
  if (n >= ((int64_t)1 << 32) / ncam + 1 || n * ncam >= ((int64_t)1 << 32)) return FSF_ERR_UNSUPPORTED;  // (values are u32)
  if ((int64_t)ncam * ((int64_t)feat_h + 1) * ((int64_t)feat_w + 1) >= ((int64_t)1 << 31)) return FSF_ERR_UNSUPPORTED;
  return FSF_OK;
}

}  // namespace fsf

using namespace fsf;

extern "C" int64_t fsf_project_gather_bilinear_backward_workspace_bytes(int64_t n, int32_t ncam, int32_t feat_h, int32_t feat_w,
                                                                        int32_t channels) {
  if (bilinear_bwd_shape_status(n, ncam, feat_h, feat_w, channels) != FSF_OK) return 0;
  return fsf_layout_bytes<BilinBwdLayout>(n * ncam, (int64_t)ncam * (feat_h + 1) * (feat_w + 1));
}

extern "C" int fsf_project_gather_bilinear_backward(const float* xyz, int64_t n, int32_t xyz_stride, const float* lidar2img, int32_t ncam,
                                                    const float* grad_out, int32_t channels, int32_t feat_h, int32_t feat_w,
                                                    int32_t channels_last, int32_t img_h, int32_t img_w, int32_t reduce_cams,
                                                    float* grad_feat, void* workspace, int64_t workspace_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (n < 0 || xyz_stride < 3 || ncam < 1 || ncam > 64 || channels < 1 || feat_h < 1 || feat_w < 1 || img_h < 1 || img_w < 1 ||
      !lidar2img || !grad_feat || (n > 0 && (!xyz || !grad_out)))
    return FSF_ERR_INVALID_ARG;
  const int rc_shape = bilinear_bwd_shape_status(n, ncam, feat_h, feat_w, channels);
  if (rc_shape != FSF_OK) return rc_shape;
  const int64_t total = n * ncam, num_cells = (int64_t)ncam * (feat_h + 1) * (feat_w + 1);
  FSF_CARVE(BilinBwdLayout, l, workspace, workspace_bytes, total, num_cells);
  const RadixScratch& s = l.sort;
  const int64_t texels = (int64_t)ncam * feat_h * feat_w;
  if (n == 0) {  // no taps: the all-zero map
    FSF_HIP_TRY(hipMemsetAsync(grad_feat, 0, (size_t)texels * channels * sizeof(float), stream));
    return FSF_OK;
  }
  BilinBwdKeyArgs ka{xyz, lidar2img, s.keys_a, s.vals_a, l.frac, total, (int)xyz_stride, (int)ncam, (int)feat_h, (int)feat_w, (int)img_h, (int)img_w};
  hipLaunchKernelGGL(bilinear_bwd_keys_kernel, dim3(fsf_stream_grid(total, 256)), dim3(256), (size_t)ncam * 12 * sizeof(float), stream, ka);
  FSF_LAUNCH_CHECK();
  int key_bits = 1;
  while (((int64_t)1 << key_bits) <= num_cells) ++key_bits;  // the sentinel NC itself is a key
  uint64_t* keys_s = nullptr;
  uint32_t* vals_s = nullptr;
  const int rc = radix_sort_pairs(s.keys_a, s.vals_a, s.keys_b, s.vals_b, s.hist, total, key_bits, &keys_s, &vals_s, stream);
  if (rc != FSF_OK) return rc;
  hipLaunchKernelGGL(bilinear_bwd_starts_kernel, dim3(fsf_stream_grid(num_cells + 1, 256)), dim3(256), 0, stream, keys_s, total, num_cells,
                     l.start);
  FSF_LAUNCH_CHECK();
  BilinBwdSumArgs sa{vals_s, l.start, l.frac, grad_out, grad_feat, texels, (int)ncam, (int)channels, (int)feat_h, (int)feat_w,
                     (int)(channels_last != 0), (int)(reduce_cams != 0)};
  const bool vec = channels % 4 == 0 && ((uintptr_t)grad_out % 16) == 0 && (!channels_last || ((uintptr_t)grad_feat % 16) == 0);
  int64_t grid = (texels + 3) / 4;
  if (grid > 65536) grid = 65536;
  if (vec)
    hipLaunchKernelGGL(bilinear_bwd_sum_kernel<4>, dim3((unsigned)grid), dim3(256), 0, stream, sa);
  else
    hipLaunchKernelGGL(bilinear_bwd_sum_kernel<1>, dim3((unsigned)grid), dim3(256), 0, stream, sa);
  FSF_LAUNCH_CHECK();
  return FSF_OK;
}
