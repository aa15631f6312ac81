// K34: the camera branch's instance-id planes painted on the device from 2-D detections — see include/fsf_hip.h and
// docs/kernels/K34_mask_paint.md.
//   fsf_mask_extents          (K34a): full-resolution u8 / bool masks [N, H, W] -> (y0, x0, h, w) of each mask's nonzero pixels,
//                                     one workgroup per mask, 16-byte loads, wave + LDS min / max reduction
//   fsf_paint_instance_masks  (K34b): an ordered object table (CSR per output plane, paint order) -> u8 or i32 planes; every
//                                     output element is written exactly once (zeros included), a resized plane's source index
//                                     floor(f32(i) * f32(scale)) is folded in
//   fsf_paint_roi_masks       (K34c): the same planes from a mask head's RoI maps [N, M, M] + boxes: K34b's tile loop with mmdet's
//                                     paste (bilinear sample of the map over the box, then a threshold) evaluated per pixel, so no
//                                     full-size mask ever exists and K34a does not run
// A pixel takes the id of the FIRST object of its plane (table order) whose mask covers it; the host planner
// (mmdet3d_plugin/datasets/mask_paint.py) puts the rows in the reference writer's paint order.
#include "common.h"

namespace fsf {

constexpr int MX_BLOCK = 256;
constexpr int MP_TILE_VECS = 16;                            // 16 lanes x 16 pixels = 256 output columns per tile row
constexpr int MP_TILE_ROWS = MX_BLOCK / MP_TILE_VECS;        // 16 rows
constexpr int MP_TILE_COLS = MP_TILE_VECS * 16;
constexpr int MP_CHUNK = MX_BLOCK;                           // objects culled per pass (a plane with more is chunked)
constexpr int MP_ROW_WORDS = 8;                              // (plane, y0, x0, h, w, pitch, ext_row, id)

// ------------------------------------------------------------------------------------------------ K34a
__device__ __forceinline__ uint32_t nonzero_bytes(uint32_t w) {  // bit b set iff byte b of w is nonzero
  return ((w & 0xffu) ? 1u : 0u) | ((w & 0xff00u) ? 2u : 0u) | ((w & 0xff0000u) ? 4u : 0u) | ((w & 0xff000000u) ? 8u : 0u);
}

__global__ void __launch_bounds__(MX_BLOCK) mask_extents_kernel(const uint8_t* __restrict__ masks, int32_t h, int32_t w,
                                                                 const int32_t* __restrict__ mask_index, int32_t* __restrict__ out,
                                                                 int64_t out_stride) {
  const int k = blockIdx.x;
  const int64_t m = mask_index ? mask_index[k] : k;
  const int64_t plane = (int64_t)h * w;
  const uint4* src = reinterpret_cast<const uint4*>(masks + m * plane);
  const int64_t nvec = plane / 16;
  int ymin = INT32_MAX, xmin = INT32_MAX, ymax = -1, xmax = -1;
  for (int64_t v = threadIdx.x; v < nvec; v += MX_BLOCK) {
    const uint4 q = src[v];
    const uint32_t bits = nonzero_bytes(q.x) | (nonzero_bytes(q.y) << 4) | (nonzero_bytes(q.z) << 8) | (nonzero_bytes(q.w) << 12);
    if (!bits) continue;
    const int64_t p0 = v * 16;
    const int64_t pf = p0 + __builtin_ctz(bits), pl = p0 + 31 - __builtin_clz(bits);
    const int yf = (int)(pf / w), yl = (int)(pl / w);
    if (yf == yl) {  // the 16 bytes lie in one row (always when w % 16 == 0)
      ymin = min(ymin, yf);
      ymax = max(ymax, yf);
      xmin = min(xmin, (int)(pf - (int64_t)yf * w));
      xmax = max(xmax, (int)(pl - (int64_t)yl * w));
    } else {
      for (uint32_t b = bits; b; b &= b - 1) {
        const int64_t p = p0 + __builtin_ctz(b);
        const int y = (int)(p / w), x = (int)(p - (int64_t)y * w);
        ymin = min(ymin, y);
        ymax = max(ymax, y);
        xmin = min(xmin, x);
        xmax = max(xmax, x);
      }
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    ymin = min(ymin, __shfl_xor(ymin, o));
    xmin = min(xmin, __shfl_xor(xmin, o));
    ymax = max(ymax, __shfl_xor(ymax, o));
    xmax = max(xmax, __shfl_xor(xmax, o));
  }
  __shared__ int red[MX_BLOCK / 64][4];
  const int wave = threadIdx.x >> 6;
  if (fsf_lane() == 0) {
    red[wave][0] = ymin;
    red[wave][1] = xmin;
    red[wave][2] = ymax;
    red[wave][3] = xmax;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < MX_BLOCK / 64; ++i) {
      ymin = min(ymin, red[i][0]);
      xmin = min(xmin, red[i][1]);
      ymax = max(ymax, red[i][2]);
      xmax = max(xmax, red[i][3]);
    }
    int32_t* o = out + (int64_t)k * out_stride;
    const bool empty = ymax < 0;
    o[0] = empty ? 0 : ymin;
    o[1] = empty ? 0 : xmin;
    o[2] = empty ? 0 : ymax - ymin + 1;
    o[3] = empty ? 0 : xmax - xmin + 1;
  }
}

// ------------------------------------------------------------------------------------------------ K34b
struct PaintObj {
  int32_t y0, x0, h, w, pitch, id;
  int64_t off;
};

__device__ __forceinline__ int src_index(int i, float scale, int n_src, bool resized) {
  if (!resized) return i;
  const int s = (int)floorf(__fmul_rn((float)i, scale));
  return min(s, n_src - 1);
}

template <typename OutT>
__global__ void __launch_bounds__(MX_BLOCK) paint_kernel(const int32_t* __restrict__ table, const int64_t* __restrict__ src_off,
                                                         const int32_t* __restrict__ plane_ptr, const int32_t* __restrict__ plane_src_hw,
                                                         const float* __restrict__ plane_scale, const int32_t* __restrict__ extents,
                                                         const uint8_t* __restrict__ masks, int32_t dst_h, int32_t dst_w,
                                                         int32_t tiles_x, OutT* __restrict__ out) {
  __shared__ PaintObj objs[MP_CHUNK];
  __shared__ int wave_count[MX_BLOCK / 64];
  const int plane = blockIdx.y;
  const int tile = blockIdx.x;
  const int ty0 = (tile / tiles_x) * MP_TILE_ROWS, tx0 = (tile % tiles_x) * MP_TILE_COLS;
  const int ty1 = min(ty0 + MP_TILE_ROWS, dst_h), tx1 = min(tx0 + MP_TILE_COLS, dst_w);
  const int src_h = plane_src_hw[2 * plane], src_w = plane_src_hw[2 * plane + 1];
  const float sy = plane_scale[2 * plane], sx = plane_scale[2 * plane + 1];
  const bool resized = src_h != dst_h || src_w != dst_w;
  // the tile's footprint in source pixels (the nearest-index maps are monotone)
  const int sy_lo = src_index(ty0, sy, src_h, resized), sy_hi = src_index(ty1 - 1, sy, src_h, resized);
  const int sx_lo = src_index(tx0, sx, src_w, resized), sx_hi = src_index(tx1 - 1, sx, src_w, resized);

  const int y = ty0 + (int)threadIdx.x / MP_TILE_VECS;
  const int x = tx0 + ((int)threadIdx.x % MP_TILE_VECS) * 16;
  const bool active = y < ty1 && x < tx1;  // dst_w % 16 == 0: a lane's 16 pixels are all inside or all outside
  const int ys = active ? src_index(y, sy, src_h, resized) : 0;
  int xs[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) xs[j] = active ? src_index(x + j, sx, src_w, resized) : 0;
  int ids[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) ids[j] = 0;
  uint32_t open = active ? 0xffffu : 0u;  // pixels not yet claimed

  const int p0 = plane_ptr[plane], p1 = plane_ptr[plane + 1];
  const int lane = fsf_lane(), wave = threadIdx.x >> 6;
  for (int c0 = p0; c0 < p1; c0 += MP_CHUNK) {
    if (!__syncthreads_or(open != 0u)) break;  // (also orders this pass's LDS writes after the previous pass's reads)
    // cull the chunk against the tile into an order-preserving LDS list
    const int r = c0 + (int)threadIdx.x;
    bool keep = false;
    PaintObj o{};
    if (r < p1) {
      const int32_t* row = table + (int64_t)r * MP_ROW_WORDS;
      const int ext = row[6];
      const int32_t* rect = ext >= 0 ? extents + (int64_t)ext * 4 : row + 1;
      o.y0 = rect[0];
      o.x0 = rect[1];
      o.h = rect[2];
      o.w = rect[3];
      o.pitch = row[5];
      o.id = row[7];
      o.off = src_off[r];
      keep = o.h > 0 && o.w > 0 && o.y0 <= sy_hi && o.y0 + o.h > sy_lo && o.x0 <= sx_hi && o.x0 + o.w > sx_lo;
    }
    const uint64_t ballot = __ballot(keep);
    if (lane == 0) wave_count[wave] = __popcll(ballot);
    __syncthreads();
    int base = 0, total = 0;
#pragma unroll
    for (int i = 0; i < MX_BLOCK / 64; ++i) {
      base += i < wave ? wave_count[i] : 0;
      total += wave_count[i];
    }
    if (keep) objs[base + __popcll(ballot & ((1ull << lane) - 1ull))] = o;
    __syncthreads();
    for (int i = 0; i < total && open; ++i) {
      const PaintObj& q = objs[i];
      if (ys < q.y0 || ys >= q.y0 + q.h) continue;
      const uint8_t* src = masks + q.off + (int64_t)ys * q.pitch;
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        if (!((open >> j) & 1u) || xs[j] < q.x0 || xs[j] >= q.x0 + q.w) continue;
        if (q.pitch == 0 || src[xs[j]] != 0) {  // pitch 0: a solid rectangle (bbox_only)
          ids[j] = q.id;
          open &= ~(1u << j);
        }
      }
    }
  }
  if (!active) return;
  OutT* dst = out + ((int64_t)plane * dst_h + y) * dst_w + x;
  if constexpr (sizeof(OutT) == 1) {
    uint32_t wv[4];
#pragma unroll
    for (int q = 0; q < 4; ++q)
      wv[q] = (uint32_t)(ids[4 * q] & 0xff) | ((uint32_t)(ids[4 * q + 1] & 0xff) << 8) | ((uint32_t)(ids[4 * q + 2] & 0xff) << 16) |
              ((uint32_t)(ids[4 * q + 3] & 0xff) << 24);
    *reinterpret_cast<uint4*>(dst) = make_uint4(wv[0], wv[1], wv[2], wv[3]);
  } else {
#pragma unroll
    for (int q = 0; q < 4; ++q) reinterpret_cast<int4*>(dst)[q] = make_int4(ids[4 * q], ids[4 * q + 1], ids[4 * q + 2], ids[4 * q + 3]);
  }
}

// ------------------------------------------------------------------------------------------------ K34c
// K34b's tile loop with the mask pasted on the fly: a row's mask is its RoI map [M, M] sampled over its box by mmdet's
// _do_paste_mask rule and thresholded (roi_cover in mmdet3d_plugin/datasets/mask_paint.py is the host specification; the library is
// built with -ffp-contract=off, so every operation below rounds once, as there).
struct RoiObj {
  int32_t y0, x0, h, w, id;
  float bx0, by0, bx1, by1;
  int64_t off;
};

__device__ __forceinline__ float texel(const float* m, int64_t i) { return m[i]; }
__device__ __forceinline__ float texel(const _Float16* m, int64_t i) { return (float)m[i]; }  // f16 -> f32 is exact

// One axis of the paste for source pixel p of a box side [lo, hi): the first tap i0 (valid only when the function returns true:
// i0 in [-1, M), so that at least one of the taps i0, i0 + 1 can lie in the map) and the weights of i0 and i0 + 1.
__device__ __forceinline__ bool roi_taps(int p, float lo, float hi, int M, int& i0, float& w0, float& w1) {
  const float g = __fdiv_rn(((float)p + 0.5f) - lo, hi - lo) * 2.0f - 1.0f;
  const float i = ((g + 1.0f) * (float)M - 1.0f) * 0.5f;
  const float f = floorf(i);
  w1 = i - f;
  w0 = 1.0f - w1;
  const bool ok = f >= -1.0f && f < (float)M;  // (false for a NaN; checked before the conversion to int)
  i0 = ok ? (int)f : 0;
  return ok;
}

template <typename OutT, typename TexT>
__global__ void __launch_bounds__(MX_BLOCK) paint_roi_kernel(const int32_t* __restrict__ table, const float* __restrict__ boxes,
                                                             const int64_t* __restrict__ roi_off, const int32_t* __restrict__ plane_ptr,
                                                             const int32_t* __restrict__ plane_src_hw, const float* __restrict__ plane_scale,
                                                             const TexT* __restrict__ rois, int32_t M, float thr, int32_t dst_h,
                                                             int32_t dst_w, int32_t tiles_x, OutT* __restrict__ out) {
  __shared__ RoiObj objs[MP_CHUNK];
  __shared__ int wave_count[MX_BLOCK / 64];
  const int plane = blockIdx.y;
  const int tile = blockIdx.x;
  const int ty0 = (tile / tiles_x) * MP_TILE_ROWS, tx0 = (tile % tiles_x) * MP_TILE_COLS;
  const int ty1 = min(ty0 + MP_TILE_ROWS, dst_h), tx1 = min(tx0 + MP_TILE_COLS, dst_w);
  const int src_h = plane_src_hw[2 * plane], src_w = plane_src_hw[2 * plane + 1];
  const float sy = plane_scale[2 * plane], sx = plane_scale[2 * plane + 1];
  const bool resized = src_h != dst_h || src_w != dst_w;
  const int sy_lo = src_index(ty0, sy, src_h, resized), sy_hi = src_index(ty1 - 1, sy, src_h, resized);
  const int sx_lo = src_index(tx0, sx, src_w, resized), sx_hi = src_index(tx1 - 1, sx, src_w, resized);

  const int y = ty0 + (int)threadIdx.x / MP_TILE_VECS;
  const int x = tx0 + ((int)threadIdx.x % MP_TILE_VECS) * 16;
  const bool active = y < ty1 && x < tx1;  // dst_w % 16 == 0: a lane's 16 pixels are all inside or all outside
  const int ys = active ? src_index(y, sy, src_h, resized) : 0;
  int xs[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) xs[j] = active ? src_index(x + j, sx, src_w, resized) : 0;
  int ids[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) ids[j] = 0;
  uint32_t open = active ? 0xffffu : 0u;  // pixels not yet claimed

  const int p0 = plane_ptr[plane], p1 = plane_ptr[plane + 1];
  const int lane = fsf_lane(), wave = threadIdx.x >> 6;
  for (int c0 = p0; c0 < p1; c0 += MP_CHUNK) {
    if (!__syncthreads_or(open != 0u)) break;  // (also orders this pass's LDS writes after the previous pass's reads)
    // cull the chunk's candidate rectangles against the tile into an order-preserving LDS list
    const int r = c0 + (int)threadIdx.x;
    bool keep = false;
    RoiObj o{};
    if (r < p1) {
      const int32_t* row = table + (int64_t)r * MP_ROW_WORDS;
      const float* box = boxes + (int64_t)r * 4;
      o.y0 = row[1];
      o.x0 = row[2];
      o.h = row[3];
      o.w = row[4];
      o.id = row[7];
      o.bx0 = box[0];
      o.by0 = box[1];
      o.bx1 = box[2];
      o.by1 = box[3];
      o.off = roi_off[r];
      keep = o.h > 0 && o.w > 0 && o.y0 <= sy_hi && o.y0 + o.h > sy_lo && o.x0 <= sx_hi && o.x0 + o.w > sx_lo;
    }
    const uint64_t ballot = __ballot(keep);
    if (lane == 0) wave_count[wave] = __popcll(ballot);
    __syncthreads();
    int base = 0, total = 0;
#pragma unroll
    for (int i = 0; i < MX_BLOCK / 64; ++i) {
      base += i < wave ? wave_count[i] : 0;
      total += wave_count[i];
    }
    if (keep) objs[base + __popcll(ballot & ((1ull << lane) - 1ull))] = o;
    __syncthreads();
    for (int i = 0; i < total && open; ++i) {
      const RoiObj& q = objs[i];
      if (ys < q.y0 || ys >= q.y0 + q.h) continue;
      // the row taps, once per (object, lane)
      int iy0;
      float wy0, wy1;
      if (!roi_taps(ys, q.by0, q.by1, M, iy0, wy0, wy1)) continue;
      const bool in_y0 = iy0 >= 0, in_y1 = iy0 + 1 < M;
      const TexT* row0 = rois + q.off + (int64_t)iy0 * M;  // dereferenced only where in_y0 / in_y1 and the column test hold
      const TexT* row1 = row0 + M;
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        if (!((open >> j) & 1u) || xs[j] < q.x0 || xs[j] >= q.x0 + q.w) continue;
        int ix0;
        float wx0, wx1;
        if (!roi_taps(xs[j], q.bx0, q.bx1, M, ix0, wx0, wx1)) continue;
        const bool in_x0 = ix0 >= 0, in_x1 = ix0 + 1 < M;
        const float t00 = in_y0 && in_x0 ? texel(row0, ix0) : 0.0f, t01 = in_y0 && in_x1 ? texel(row0, ix0 + 1) : 0.0f;
        const float t10 = in_y1 && in_x0 ? texel(row1, ix0) : 0.0f, t11 = in_y1 && in_x1 ? texel(row1, ix0 + 1) : 0.0f;
        float v = t00 * (wx0 * wy0);
        v = v + t01 * (wx1 * wy0);
        v = v + t10 * (wx0 * wy1);
        v = v + t11 * (wx1 * wy1);
        if (v >= thr) {  // (false for a NaN)
          ids[j] = q.id;
          open &= ~(1u << j);
        }
      }
    }
  }
  if (!active) return;
  OutT* dst = out + ((int64_t)plane * dst_h + y) * dst_w + x;
  if constexpr (sizeof(OutT) == 1) {
    uint32_t wv[4];
#pragma unroll
    for (int q = 0; q < 4; ++q)
      wv[q] = (uint32_t)(ids[4 * q] & 0xff) | ((uint32_t)(ids[4 * q + 1] & 0xff) << 8) | ((uint32_t)(ids[4 * q + 2] & 0xff) << 16) |
              ((uint32_t)(ids[4 * q + 3] & 0xff) << 24);
    *reinterpret_cast<uint4*>(dst) = make_uint4(wv[0], wv[1], wv[2], wv[3]);
  } else {
#pragma unroll
    for (int q = 0; q < 4; ++q) reinterpret_cast<int4*>(dst)[q] = make_int4(ids[4 * q], ids[4 * q + 1], ids[4 * q + 2], ids[4 * q + 3]);
  }
}

template <typename OutT, typename TexT>
static void launch_paint_roi(dim3 grid, hipStream_t stream, const int32_t* table, const float* boxes, const int64_t* roi_off,
                             const int32_t* plane_ptr, const int32_t* plane_src_hw, const float* plane_scale, const void* rois, int32_t M,
                             float thr, int32_t dst_h, int32_t dst_w, int32_t tiles_x, void* out) {
  hipLaunchKernelGGL((paint_roi_kernel<OutT, TexT>), grid, dim3(MX_BLOCK), 0, stream, table, boxes, roi_off, plane_ptr, plane_src_hw,
                     plane_scale, (const TexT*)rois, M, thr, dst_h, dst_w, tiles_x, (OutT*)out);
}

}  // namespace fsf

using namespace fsf;

extern "C" int fsf_mask_extents(const uint8_t* masks, int64_t n_masks, int32_t h, int32_t w, const int32_t* mask_index, int64_t n_out,
                                int32_t* out, int64_t out_stride, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (n_masks < 0 || n_out < 0 || h < 1 || w < 1 || out_stride < 4) return FSF_ERR_INVALID_ARG;
  if (!mask_index && n_out > n_masks) return FSF_ERR_INVALID_ARG;
  if (n_out == 0) return FSF_OK;
  if (!masks || !out) return FSF_ERR_INVALID_ARG;
  if (((int64_t)h * w) % 16 != 0 || ((uintptr_t)masks & 15u) != 0 || n_out >= ((int64_t)1 << 31)) return FSF_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(mask_extents_kernel, dim3((unsigned)n_out), dim3(MX_BLOCK), 0, stream, masks, h, w, mask_index, out, out_stride);
  FSF_LAUNCH_CHECK();
  return FSF_OK;
}

extern "C" int fsf_paint_instance_masks(const int32_t* table, const int64_t* src_off, int64_t n_rows, const int32_t* plane_ptr,
                                        const int32_t* plane_src_hw, const float* plane_scale, int32_t num_planes,
                                        const int32_t* extents, const uint8_t* masks, int32_t dst_h, int32_t dst_w, int32_t out_elem_bytes,
                                        void* out, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (n_rows < 0 || num_planes < 0 || dst_h < 1 || dst_w < 1 || (out_elem_bytes != 1 && out_elem_bytes != 4)) return FSF_ERR_INVALID_ARG;
  if (num_planes == 0) return FSF_OK;
  if (!plane_ptr || !plane_src_hw || !plane_scale || !out || (n_rows > 0 && (!table || !src_off))) return FSF_ERR_INVALID_ARG;
  if (dst_w % 16 != 0 || ((uintptr_t)out & 15u) != 0 || num_planes > 65535 || n_rows >= ((int64_t)1 << 31)) return FSF_ERR_UNSUPPORTED;
  const int tiles_x = fsf_cdiv(dst_w, MP_TILE_COLS), tiles_y = fsf_cdiv(dst_h, MP_TILE_ROWS);
  const dim3 grid((unsigned)(tiles_x * tiles_y), (unsigned)num_planes);
  if (out_elem_bytes == 1)
    hipLaunchKernelGGL(paint_kernel<uint8_t>, grid, dim3(MX_BLOCK), 0, stream, table, src_off, plane_ptr, plane_src_hw, plane_scale,
                       extents, masks, dst_h, dst_w, tiles_x, (uint8_t*)out);
  else
    hipLaunchKernelGGL(paint_kernel<int32_t>, grid, dim3(MX_BLOCK), 0, stream, table, src_off, plane_ptr, plane_src_hw, plane_scale,
                       extents, masks, dst_h, dst_w, tiles_x, (int32_t*)out);
  FSF_LAUNCH_CHECK();
  return FSF_OK;
}

extern "C" int fsf_paint_roi_masks(const int32_t* table, const float* boxes, const int64_t* roi_off, int64_t n_rows,
                                   const int32_t* plane_ptr, const int32_t* plane_src_hw, const float* plane_scale, int32_t num_planes,
                                   const void* rois, int32_t roi_size, int32_t roi_elem_bytes, float thr, int32_t dst_h, int32_t dst_w,
                                   int32_t out_elem_bytes, void* out, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (n_rows < 0 || num_planes < 0 || dst_h < 1 || dst_w < 1 || (out_elem_bytes != 1 && out_elem_bytes != 4)) return FSF_ERR_INVALID_ARG;
  if (roi_size < 1 || roi_size > 64 || (roi_elem_bytes != 2 && roi_elem_bytes != 4) || !(thr > 0.0f)) return FSF_ERR_INVALID_ARG;
  if (num_planes == 0) return FSF_OK;
  if (!plane_ptr || !plane_src_hw || !plane_scale || !out || (n_rows > 0 && (!table || !boxes || !roi_off || !rois)))
    return FSF_ERR_INVALID_ARG;
  if (dst_w % 16 != 0 || ((uintptr_t)out & 15u) != 0 || num_planes > 65535 || n_rows >= ((int64_t)1 << 31)) return FSF_ERR_UNSUPPORTED;
  if (((uintptr_t)rois & (uintptr_t)(roi_elem_bytes - 1)) != 0) return FSF_ERR_UNSUPPORTED;
  const int tiles_x = fsf_cdiv(dst_w, MP_TILE_COLS), tiles_y = fsf_cdiv(dst_h, MP_TILE_ROWS);
  const dim3 grid((unsigned)(tiles_x * tiles_y), (unsigned)num_planes);
  auto launch = out_elem_bytes == 1 ? (roi_elem_bytes == 4 ? launch_paint_roi<uint8_t, float> : launch_paint_roi<uint8_t, _Float16>)
                                    : (roi_elem_bytes == 4 ? launch_paint_roi<int32_t, float> : launch_paint_roi<int32_t, _Float16>);
  launch(grid, stream, table, boxes, roi_off, plane_ptr, plane_src_hw, plane_scale, rois, roi_size, thr, dst_h, dst_w, tiles_x, out);
  FSF_LAUNCH_CHECK();
  return FSF_OK;
}
