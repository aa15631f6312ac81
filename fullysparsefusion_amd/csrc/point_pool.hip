// K17: dynamic point pooling — which points fall inside which (enlarged) rotated RoI, with per-point box-frame geometry.
// Replaces: TorchEx dynamic_point_pool_ext.forward [UNVENDORED], called from
//   projects/mmdet3d_plugin/ops/dynamic_point_pool_op.py:27-32 by DynamicPointROIExtractor
//   (projects/mmdet3d_plugin/models/roi_heads/roi_extractors/dynamic_point_roi_extractor.py:54-59).
// Upstream: grid (ceil(P/256), R) brute force, `cnt = atomicAdd(&inbox_counter[box], 1)` (drop if >= max_inbox) and
//   `slot = atomicAdd(&global_counter, 1)` (drop if >= max_all): WHICH points survive the caps and the order of the
//   output rows depend on the atomics.  Here the result is canonical: rows in ascending (roi, point index) order, a
//   RoI keeps its first `max_inbox` points by index, the output keeps the first `max_all` rows — count, prefix, fill
//   (three passes over the same test), no atomics.
// Box convention (mmdet3d 0.x LiDAR): (cx, cy, cz_bottom, w, l, h, rz); local frame rotated by rz + pi/2, local_x along
//   the length l, local_y along the width w (pinned by dynamic_point_roi_extractor.py:83-92).
// The 13 floats per row: x, y, z | local_x, local_y, local_z (z - box centre) | distances to the six faces
//   (lx + l/2, ly + w/2, lz + h/2, l/2 - lx, w/2 - ly, h/2 - lz) | is_in_margin (1 = only inside the enlarged box).
// Work: thread = RoI, workgroup = 256 RoIs x one tile of 2048 points staged in LDS (every lane reads the same point:
//   LDS broadcast); a cheap enlarged-radius test in the xy-plane rejects almost every pair before the rotation.
#include <stdlib.h>

#include "common.h"
#include "radix_sort.h"
#include "scan.h"

namespace fsf {
extern std::atomic<int64_t> g_opt_pool_brute;  // status.hip

constexpr int PP_TILE = 2048;
constexpr int PP_FEAT = 13;

struct PoolArgs {
  const float* rois;
  const float* pts;
  const int64_t* pts_batch;
  int64_t n_rois, n_pts;
  int roi_stride, box_col, batch_col, pts_stride;
  float ew, el, eh;
  int max_inbox;
  int64_t max_all;
  uint32_t* cnt;       // [pt_tiles][n_rois]
  uint32_t* roi_total; // [n_rois]   min(#in box, max_inbox)
  uint32_t* roi_off;   // [n_rois]   exclusive prefix of roi_total
  int64_t* out_pts;
  int64_t* out_roi;
  float* out_feat;
  // The count pass runs in chunks of RoI groups (1, 2, 4, ... groups of 256 RoIs): the output keeps only the first
  // max_all rows in (roi, point) order, so once the chunks before this one have reached that many in-box points the rest
  // of the RoIs cannot contribute a row — their workgroups return at once and their totals stay 0.  (Bench frame: 10.6 k
  // small RoIs with 5-10 points each reach max_all = 50 000 only in the fifth chunk, so the count pass goes 649 -> 579 us;
  // well-populated RoIs reach it in the first groups.)
  int group0;             // first RoI group of this launch
  int chunk;              // index of this chunk
  uint32_t* chunk_total;  // [32] in-box points (capped per RoI) of every chunk so far; chunk i adds into [i]
};

__device__ __forceinline__ bool pool_cap_reached(const PoolArgs& a) {
  uint64_t before = 0;
  for (int i = 0; i < a.chunk; ++i) before += a.chunk_total[i];
  return before >= (uint64_t)a.max_all;
}

struct PoolBox {
  float cx, cy, cz, hw, hl, hh, lhw, lhl, lhh, cosa, sina, r2;
  int batch;
};

__device__ __forceinline__ PoolBox load_box(const PoolArgs& a, int64_t r) {
  const float* row = a.rois + r * a.roi_stride;
  const float* b = row + a.box_col;
  PoolBox k;
  const float w = b[3], l = b[4], h = b[5];
  k.cx = b[0];
  k.cy = b[1];
  k.cz = b[2] + h * 0.5f;  // bottom centre -> centre
  k.hw = w * 0.5f;
  k.hl = l * 0.5f;
  k.hh = h * 0.5f;
  k.lhw = (w + a.ew) * 0.5f;
  k.lhl = (l + a.el) * 0.5f;
  k.lhh = (h + a.eh) * 0.5f;
  const float rot = b[6] + 1.57079632679489661923f;
  k.cosa = cosf(rot);
  k.sina = sinf(rot);
  k.r2 = (k.lhw * k.lhw + k.lhl * k.lhl) * 1.0001f + 1e-6f;  // conservative pre-test only
  k.batch = a.batch_col >= 0 ? (int)row[a.batch_col] : 0;
  return k;
}

// 0 = outside, 1 = inside the box, 2 = inside the enlarged box only
__device__ __forceinline__ int pool_test(const PoolBox& k, float x, float y, float z, float& lx, float& ly, float& lz) {
  const float dx = x - k.cx, dy = y - k.cy;
  if (dx * dx + dy * dy > k.r2) return 0;  // rejects almost every pair: keep it first
  lz = z - k.cz;
  if (!(fabsf(lz) <= k.lhh)) return 0;  // (written so that a NaN z is outside, as NaN x / y are below)
  lx = dx * k.cosa + dy * (-k.sina);
  ly = dx * k.sina + dy * k.cosa;
  const bool in_large = (lx > -k.lhl) & (lx < k.lhl) & (ly > -k.lhw) & (ly < k.lhw);
  if (!in_large) return 0;
  const bool in_box = (lx > -k.hl) & (lx < k.hl) & (ly > -k.hw) & (ly < k.hw) & (fabsf(lz) <= k.hh);
  return in_box ? 1 : 2;
}

template <bool FILL>
__global__ void __launch_bounds__(256) pool_pass_kernel(PoolArgs a) {
  __shared__ float4 sp[PP_TILE];       // x, y, z, batch index (exact in fp32) of the tile's points that can matter
  __shared__ uint16_t sj[PP_TILE];     // their position in the tile
  __shared__ float sred[4][4];
  __shared__ int swave[4];
  __shared__ int s_ns;
  const int64_t r = ((int64_t)blockIdx.x + a.group0) * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (FILL) {
    // rows past the global cap are never written: when the whole RoI tile starts beyond it there is nothing to do
    // (with max_all_pts = 50000 and thousands of queries that is nearly every tile)
    const int64_t r_first = ((int64_t)blockIdx.x + a.group0) * 256;
    if ((int64_t)a.roi_off[r_first] >= a.max_all) return;
  } else if (pool_cap_reached(a)) {
    return;
  }
  // This workgroup's 256 RoIs.  Queries arrive cluster by cluster in voxel order, so consecutive RoIs are close in
  // space: the bounding box of their (enlarged) circles is small, and only the tile's points inside it are kept —
  // an order-preserving compaction, so ranks and output order are unchanged.  Unsorted RoIs just keep every point.
  const bool has_roi = r < a.n_rois;
  PoolBox k = load_box(a, has_roi ? r : a.n_rois - 1);
  const float rad = sqrtf(k.r2);
  float bx0 = k.cx - rad, bx1 = k.cx + rad, by0 = k.cy - rad, by1 = k.cy + rad;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    bx0 = fminf(bx0, __shfl_xor(bx0, o));
    bx1 = fmaxf(bx1, __shfl_xor(bx1, o));
    by0 = fminf(by0, __shfl_xor(by0, o));
    by1 = fmaxf(by1, __shfl_xor(by1, o));
  }
  if (lane == 0) {
    sred[wave][0] = bx0;
    sred[wave][1] = bx1;
    sred[wave][2] = by0;
    sred[wave][3] = by1;
  }
  if (threadIdx.x == 0) s_ns = 0;
  __syncthreads();
  bx0 = fminf(fminf(sred[0][0], sred[1][0]), fminf(sred[2][0], sred[3][0]));
  bx1 = fmaxf(fmaxf(sred[0][1], sred[1][1]), fmaxf(sred[2][1], sred[3][1]));
  by0 = fminf(fminf(sred[0][2], sred[1][2]), fminf(sred[2][2], sred[3][2]));
  by1 = fmaxf(fmaxf(sred[0][3], sred[1][3]), fmaxf(sred[2][3], sred[3][3]));
  const int64_t p0 = (int64_t)blockIdx.y * PP_TILE;
  const int tile_n = (int)min((int64_t)PP_TILE, a.n_pts - p0);
  for (int j0 = 0; j0 < tile_n; j0 += 256) {  // 256 points per round, appended in index order
    const int j = j0 + threadIdx.x;
    float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
    bool keep = false;
    if (j < tile_n) {
      const float* p = a.pts + (p0 + j) * a.pts_stride;
      q = make_float4(p[0], p[1], p[2], a.pts_batch ? (float)a.pts_batch[p0 + j] : 0.0f);
      keep = (q.x >= bx0) & (q.x <= bx1) & (q.y >= by0) & (q.y <= by1);
    }
    const uint64_t bal = __ballot(keep);
    if (lane == 0) swave[wave] = __popcll(bal);
    __syncthreads();
    int base = s_ns;
    for (int w = 0; w < wave; ++w) base += swave[w];
    if (keep) {
      const int pos = base + __popcll(bal & ((1ull << lane) - 1ull));
      sp[pos] = q;
      sj[pos] = (uint16_t)j;
    }
    __syncthreads();
    if (threadIdx.x == 0) s_ns += swave[0] + swave[1] + swave[2] + swave[3];
    __syncthreads();
  }
  const int ns = s_ns;
  if (!has_roi) return;
  const float kbatch = (float)k.batch;
  uint32_t* my_cnt = a.cnt + (int64_t)blockIdx.y * a.n_rois + r;
  uint32_t rank = FILL ? *my_cnt : 0u;  // after the prefix pass: in-box points of this RoI in earlier tiles
  const uint32_t base = FILL ? a.roi_off[r] : 0u;
  if (FILL && (rank >= (uint32_t)a.max_inbox || (int64_t)base + rank >= a.max_all)) return;  // caps already reached
#pragma unroll 4
  for (int i = 0; i < ns; ++i) {
    const float4 q = sp[i];
    float lx, ly, lz;
    const int flag = (q.w == kbatch) ? pool_test(k, q.x, q.y, q.z, lx, ly, lz) : 0;
    if (flag) {
      if (FILL) {
        const int64_t slot = (int64_t)base + rank;
        if (rank < (uint32_t)a.max_inbox && slot < a.max_all) {
          a.out_pts[slot] = p0 + sj[i];
          a.out_roi[slot] = r;
          float* f = a.out_feat + slot * PP_FEAT;
          f[0] = q.x;
          f[1] = q.y;
          f[2] = q.z;
          f[3] = lx;
          f[4] = ly;
          f[5] = lz;
          f[6] = lx + k.hl;
          f[7] = ly + k.hw;
          f[8] = lz + k.hh;
          f[9] = k.hl - lx;
          f[10] = k.hw - ly;
          f[11] = k.hh - lz;
          f[12] = flag == 2 ? 1.0f : 0.0f;
        }
      }
      ++rank;
    }
  }
  if (!FILL) *my_cnt = rank;
}

// per RoI: counts per point tile -> exclusive prefix over tiles (in place), capped total
__global__ void __launch_bounds__(256) pool_prefix_kernel(PoolArgs a, int pt_tiles) {
  const int64_t r = ((int64_t)blockIdx.x + a.group0) * 256 + threadIdx.x;
  if (pool_cap_reached(a)) return;  // (roi_total stays 0: the RoI's rows would lie past max_all)
  uint32_t tot = 0;
  if (r < a.n_rois) {
    uint32_t run = 0;
    for (int t = 0; t < pt_tiles; ++t) {
      uint32_t* c = a.cnt + (int64_t)t * a.n_rois + r;
      const uint32_t v = *c;
      *c = run;
      run += v;
    }
    tot = min(run, (uint32_t)a.max_inbox);
    a.roi_total[r] = tot;
  }
  // this chunk's total for the chunks after it (a sum of integers: the order of the atomics does not matter)
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) tot += __shfl_xor(tot, o);
  if ((threadIdx.x & 63) == 0 && tot) atomicAdd(&a.chunk_total[a.chunk], tot);
}

struct PoolScanIn {
  const uint32_t* v;
  __device__ uint32_t operator()(int64_t i) const { return v[i]; }
};
struct PoolScanOut {
  uint32_t* off;
  __device__ void operator()(int64_t i, uint32_t excl, uint32_t) const { off[i] = excl; }
};

// ---- the binned path (default): P x R tests only where they can succeed -------------------------------------------------
// The brute-force passes above cost P x R pair tests behind a circle pre-test and run as a few hundred latency-bound
// workgroups (10.6 k RoIs x 3.1e5 points: 1.06 ms).  Here the points are sorted ONCE by BEV cell (1 m cells, stable radix sort:
// a cell's points stay in ascending index order), and a wave per RoI walks only the cells under its enlarged circle.  The result
// is the same canonical list: a RoI's hits are gathered in LDS, sorted by point index (bitonic, one wave) and cut at max_inbox.
// A RoI with more hits than the LDS list holds (a bus-sized box on the dense ground near the sensor) first narrows the point-index
// range that contains its first max_inbox hits (histogram of the hits' indices over 1024 ranges, at most twice) and then gathers
// only those.  Same pool_test, same features, same caps, same order as the brute-force passes (tests compare the two bit for bit).
constexpr int PB_BITS = 10;                 // cells per axis: 1024 x 1024 around the origin, the border cells take everything beyond
constexpr float PB_INV_CELL = 1.0f;         // 1 / (1 m): +-512 m
constexpr int PB_NCELL = 1 << (2 * PB_BITS);
constexpr int PB_CAP = 1024;                // hits per RoI sorted in LDS (>= max_inbox)
constexpr int PB_BINS = 1024;               // index-range bins of the selection pass for RoIs with more hits than that

__device__ __forceinline__ int pb_coord(float v) {
  float f = floorf(v * PB_INV_CELL) + (float)(1 << (PB_BITS - 1));
  f = fminf(fmaxf(f, 0.0f), (float)((1 << PB_BITS) - 1));  // (NaN -> 0: fmaxf returns the other operand)
  return (int)f;
}

__global__ void __launch_bounds__(256) pb_keys_kernel(const float* __restrict__ pts, int64_t n, int stride, uint64_t* keys, uint32_t* vals) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const float* p = pts + i * stride;
    keys[i] = (uint64_t)((pb_coord(p[1]) << PB_BITS) | pb_coord(p[0]));
    vals[i] = (uint32_t)i;
  }
}

// cell -> [start, end) of its points in the sorted order (tables zeroed beforehand: an empty cell is [0, 0)), and the points
// themselves in that order (x, y, z, batch index): a RoI's candidates are a few contiguous runs of 16-byte records
__global__ void __launch_bounds__(256)
    pb_cells_kernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ order, int64_t n, const float* __restrict__ pts, int stride,
                    const int64_t* __restrict__ pts_batch, uint32_t* cell_start, uint32_t* cell_end, float4* sorted) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const uint64_t k = keys[i];
    if (i == 0 || keys[i - 1] != k) cell_start[k] = (uint32_t)i;
    if (i == n - 1 || keys[i + 1] != k) cell_end[k] = (uint32_t)(i + 1);
    const uint32_t pi = order[i];
    const float* p = pts + (int64_t)pi * stride;
    sorted[i] = make_float4(p[0], p[1], p[2], pts_batch ? (float)pts_batch[pi] : 0.0f);
  }
}

struct PoolBinArgs {
  PoolArgs a;
  const uint32_t* order;       // point indices sorted by cell (ascending inside a cell)
  const float4* sorted;        // the points in that order
  const uint32_t* cell_start;
  const uint32_t* cell_end;
  uint32_t* hits_full;         // [n_rois] hits of the RoI before the max_inbox cut (PB_CAP + 1: more than the list holds)
};

// wave-wide walk over the candidate points of box k, 4 x 64 per round (four loads in flight per lane): f(point index, hit flag
// 0/1/2) is called by every lane for each of the round's four 64-candidate groups in order (flag 0 past the cell's end and for
// misses) and returns false (wave-uniform) to stop
template <typename F>
__device__ __forceinline__ void pb_for_candidates(const PoolBinArgs& b, const PoolBox& k, int lane, F&& f) {
  const float rad = sqrtf(k.r2);
  const int cx0 = pb_coord(k.cx - rad), cx1 = pb_coord(k.cx + rad), cy0 = pb_coord(k.cy - rad), cy1 = pb_coord(k.cy + rad);
  const float kbatch = (float)k.batch;
  // a box whose circle covers more than 1024 cells (or is not finite) walks the whole sorted array once instead of the table
  const bool whole = !((cx1 - cx0 + 1) * (cy1 - cy0 + 1) <= 1024) || !(rad == rad);
  const int ny = whole ? 1 : cy1 - cy0 + 1, nx = whole ? 1 : cx1 - cx0 + 1;
  for (int iy = 0; iy < ny; ++iy) {
    // a row of cells is one contiguous run of the sorted array (keys = y-major): walk [start of the first non-empty, end of the last)
    uint32_t s = whole ? 0u : 0xffffffffu, e = whole ? (uint32_t)b.a.n_pts : 0u;
    if (!whole) {
      const int key0 = ((cy0 + iy) << PB_BITS) | cx0;
      for (int ix = lane; ix < nx; ix += 64) {
        const uint32_t cs = b.cell_start[key0 + ix], ce = b.cell_end[key0 + ix];
        if (ce > cs) {
          s = min(s, cs);
          e = max(e, ce);
        }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        s = min(s, (uint32_t)__shfl_xor((int)s, o));
        e = max(e, (uint32_t)__shfl_xor((int)e, o));
      }
    }
    for (uint32_t j0 = s; j0 < e; j0 += 256) {
      float4 q[4];
      uint32_t pi[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const uint32_t j = j0 + 64 * u + lane;
        const uint32_t jc = j < e ? j : s;
        q[u] = b.sorted[jc];
        pi[u] = b.order[jc];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (j0 + 64 * u >= e) break;  // (uniform)
        const uint32_t j = j0 + 64 * u + lane;
        float lx, ly, lz;
        const int flag = (j < e && q[u].w == kbatch) ? pool_test(k, q[u].x, q[u].y, q[u].z, lx, ly, lz) : 0;
        if (!f(pi[u], flag)) return;
      }
    }
  }
}

__global__ void __launch_bounds__(256) pb_count_kernel(PoolBinArgs b) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= b.a.n_rois) return;
  const PoolBox k = load_box(b.a, r);
  uint32_t h = 0;
  pb_for_candidates(b, k, lane, [&](uint32_t, int flag) {
    h += (uint32_t)__popcll(__ballot(flag != 0));
    return h <= (uint32_t)PB_CAP;  // more than the list holds: the fill pass selects by index range, the exact number is not needed
  });
  if (lane == 0) {
    b.hits_full[r] = h <= (uint32_t)PB_CAP ? h : (uint32_t)PB_CAP + 1u;
    b.a.roi_total[r] = h < (uint32_t)b.a.max_inbox ? h : (uint32_t)b.a.max_inbox;
  }
}

__device__ __forceinline__ void pb_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ void pb_write_row(const PoolArgs& a, const PoolBox& k, int64_t slot, int64_t r, uint32_t pi) {
  const float* p = a.pts + (int64_t)pi * a.pts_stride;
  const float x = p[0], y = p[1], z = p[2];
  float lx, ly, lz;
  const int flag = pool_test(k, x, y, z, lx, ly, lz);
  a.out_pts[slot] = (int64_t)pi;
  a.out_roi[slot] = r;
  float* f = a.out_feat + slot * PP_FEAT;
  f[0] = x; f[1] = y; f[2] = z;
  f[3] = lx; f[4] = ly; f[5] = lz;
  f[6] = lx + k.hl; f[7] = ly + k.hw; f[8] = lz + k.hh;
  f[9] = k.hl - lx; f[10] = k.hw - ly; f[11] = k.hh - lz;
  f[12] = flag == 2 ? 1.0f : 0.0f;
}

__global__ void __launch_bounds__(256) pb_fill_kernel(PoolBinArgs b) {
  __shared__ uint32_t s_list[4][PB_CAP];
  __shared__ uint32_t s_hist[4][PB_BINS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t r = (int64_t)blockIdx.x * 4 + wave;
  if (r >= b.a.n_rois) return;
  const uint32_t base = b.a.roi_off[r];
  const uint32_t keep = b.a.roi_total[r];
  if (keep == 0 || (int64_t)base >= b.a.max_all) return;  // (wave-uniform)
  const PoolBox k = load_box(b.a, r);
  uint32_t* list = s_list[wave];
  uint32_t limit = 0xffffffffu;  // collect the hits of point index < limit
  if (b.hits_full[r] > (uint32_t)PB_CAP) {
    // More hits than the list holds: find an index limit below which at least `keep` (= max_inbox) and at most PB_CAP hits lie —
    // histogram of the hits' indices over PB_BINS equal ranges of [lo, hi), prefix, the range where the count crosses `keep`;
    // repeat inside that range while it alone holds too many.
    uint32_t* hist = s_hist[wave];
    uint32_t lo = 0, hi = (uint32_t)b.a.n_pts, below = 0;  // `below` hits lie under lo
    for (;;) {
      const uint32_t width = (hi - lo + PB_BINS - 1) / PB_BINS;
      for (int i = lane; i < PB_BINS; i += 64) hist[i] = 0;
      pb_wave_sync();
      pb_for_candidates(b, k, lane, [&](uint32_t pi, int flag) {
        if (flag != 0 && pi >= lo && pi < hi) atomicAdd(&hist[(pi - lo) / width], 1u);
        return true;
      });
      pb_wave_sync();
      // first bin where the running count reaches `keep`: lane l sums bins [16 l, 16 l + 16)
      uint32_t mine = 0;
      for (int i = 0; i < PB_BINS / 64; ++i) mine += hist[lane * (PB_BINS / 64) + i];
      uint32_t incl = mine;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const uint32_t v = (uint32_t)__shfl_up((int)incl, o);
        if (lane >= o) incl += v;
      }
      const uint64_t reach = __ballot(below + incl >= keep);
      const int wl = __builtin_ctzll(reach);  // (reach != 0: the RoI has more than PB_CAP >= keep hits)
      uint32_t run = below + (uint32_t)__shfl((int)(incl - mine), wl);
      int bin = wl * (PB_BINS / 64);
      for (;; ++bin) {  // (wave-uniform walk over the 16 bins of lane wl)
        const uint32_t c = hist[bin];
        if (run + c >= keep) break;
        run += c;
      }
      const uint32_t c = hist[bin];
      const uint32_t bin_lo = lo + (uint32_t)bin * width, bin_hi = min(hi, bin_lo + width);
      if (run + c <= (uint32_t)PB_CAP || width == 1) {  // (width 1: one point per bin, c <= 1)
        limit = bin_hi;
        break;
      }
      lo = bin_lo;
      hi = bin_hi;
      below = run;
      pb_wave_sync();
    }
  }
  uint32_t n_l = 0;
  pb_for_candidates(b, k, lane, [&](uint32_t pi, int flag) {
    const bool hit = flag != 0 && pi < limit;
    const uint64_t bal = __ballot(hit);
    if (hit) list[n_l + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull))] = pi;
    n_l += (uint32_t)__popcll(bal);
    return true;
  });
  uint32_t np2 = 64;
  while (np2 < n_l) np2 <<= 1;
  for (uint32_t i = n_l + lane; i < np2; i += 64) list[i] = 0xffffffffu;
  pb_wave_sync();
  for (uint32_t kk = 2; kk <= np2; kk <<= 1)
    for (uint32_t j = kk >> 1; j > 0; j >>= 1) {
      for (uint32_t i = lane; i < np2; i += 64) {
        const uint32_t ixj = i ^ j;
        if (ixj > i) {
          const uint32_t va = list[i], vb = list[ixj];
          const bool up = (i & kk) == 0;
          if ((va > vb) == up) {
            list[i] = vb;
            list[ixj] = va;
          }
        }
      }
      pb_wave_sync();
    }
  const uint32_t n_out = n_l < keep ? n_l : keep;
  for (uint32_t t = lane; t < n_out; t += 64) {
    const int64_t slot = (int64_t)base + t;
    if (slot >= b.a.max_all) break;
    pb_write_row(b.a, k, slot, r, list[t]);
  }
}

__global__ void pool_count_kernel(const uint32_t* total, int64_t max_all, int64_t* count_dev) {
  const int64_t t = (int64_t)*total;
  *count_dev = t < max_all ? t : max_all;
}

}  // namespace fsf

using namespace fsf;

struct PoolLayout {
  int pt_tiles;
  int64_t r1;
  uint32_t *cnt, *roi_total, *roi_off, *tile_sums, *total;
  int64_t* count_tmp;
  uint32_t* chunk_total;
  // the binned path only (`binned`): the sort, the cell tables and the sorted points
  uint32_t* hits_full = nullptr;
  RadixScratch sort;
  // [sort.hist | cell_start | cell_end | the scan's tile words] are consecutive: ONE memset instead of four
  uint32_t *cell_start = nullptr, *cell_end = nullptr, *tile_sums_b = nullptr;
  size_t zero_bytes = 0;
  float4* sorted = nullptr;
  PoolLayout(FsfArena& arena, int64_t n_pts, int64_t n_rois, bool binned)
      : pt_tiles(n_pts > 0 ? fsf_cdiv(n_pts, PP_TILE) : 1), r1(n_rois > 0 ? n_rois : 1), cnt(arena.take<uint32_t>((int64_t)pt_tiles * r1)),
        roi_total(arena.take<uint32_t>(r1)), roi_off(arena.take<uint32_t>(r1)), tile_sums(arena.take<uint32_t>(scan_num_tiles(r1))),
        total(arena.take<uint32_t>(1)), count_tmp(arena.take<int64_t>(1)), chunk_total(arena.take<uint32_t>(32)),
        hits_full(binned ? arena.take<uint32_t>(r1) : nullptr), sort(binned ? RadixScratch(arena, n_pts) : RadixScratch()) {
    if (!binned) return;
    cell_start = arena.take<uint32_t>(PB_NCELL);
    cell_end = arena.take<uint32_t>(PB_NCELL);
    tile_sums_b = arena.take<uint32_t>(scan_num_tiles(r1));
    zero_bytes = (size_t)(arena.offset() - sort.hist_at);
    sorted = arena.take<float4>(n_pts);
  }
};

extern "C" int64_t fsf_dynamic_point_pool_workspace_bytes(int64_t n_pts, int64_t n_rois) {
  return fsf_layout_bytes<PoolLayout>(n_pts, n_rois, true);
}

extern "C" int fsf_dynamic_point_pool(const float* rois, int64_t n_rois, int32_t roi_stride, int32_t box_col,
                                      int32_t batch_col, const float* pts, int64_t n_pts, int32_t pts_stride,
                                      const int64_t* pts_batch, const float extra_wlh[3], int32_t max_inbox_point,
                                      int64_t max_all_pts, int64_t* out_pts_idx, int64_t* out_roi_idx, float* out_pts_feats,
                                      int64_t* count_dev, int64_t* count_host, void* workspace, int64_t workspace_bytes,
                                      void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (n_rois < 0 || n_pts < 0 || roi_stride < 7 || box_col < 0 || box_col + 7 > roi_stride || batch_col >= roi_stride ||
      pts_stride < 3 || !extra_wlh || max_inbox_point < 1 || max_all_pts < 1 || !out_pts_idx || !out_roi_idx ||
      !out_pts_feats || (!count_dev && !count_host) || (n_rois > 0 && !rois) || (n_pts > 0 && !pts))
    return FSF_ERR_INVALID_ARG;
  if (n_pts >= ((int64_t)1 << 31) || n_rois >= ((int64_t)1 << 31)) return FSF_ERR_UNSUPPORTED;
  const bool brute = g_opt_pool_brute.load(std::memory_order_relaxed) != 0;  // (fsf_set_option: tests compare the two paths in one process)
  FSF_CARVE(PoolLayout, l, workspace, workspace_bytes, n_pts, n_rois, !brute && max_inbox_point <= PB_CAP);
  int64_t* cdev = count_dev ? count_dev : l.count_tmp;
  if (n_rois == 0 || n_pts == 0) {
    FSF_HIP_TRY(hipMemsetAsync(cdev, 0, sizeof(int64_t), stream));
  } else {
    PoolArgs a{rois, pts, pts_batch, n_rois, n_pts, (int)roi_stride, (int)box_col, (int)batch_col, (int)pts_stride,
               extra_wlh[0], extra_wlh[1], extra_wlh[2], (int)max_inbox_point, max_all_pts, l.cnt, l.roi_total, l.roi_off,
               out_pts_idx, out_roi_idx, out_pts_feats, 0, 0, l.chunk_total};
    if (!brute && max_inbox_point <= PB_CAP) {
      const RadixScratch& s = l.sort;
      FSF_HIP_TRY(hipMemsetAsync(s.hist, 0, l.zero_bytes, stream));
      hipLaunchKernelGGL(pb_keys_kernel, dim3((unsigned)fsf_stream_grid(n_pts, 256)), dim3(256), 0, stream, pts, n_pts, (int)pts_stride,
                         s.keys_a, s.vals_a);
      uint64_t* keys = nullptr;
      uint32_t* order = nullptr;
      int rc = radix_sort_pairs(s.keys_a, s.vals_a, s.keys_b, s.vals_b, s.hist, n_pts, 2 * PB_BITS, &keys, &order, stream, true);
      if (rc != FSF_OK) return rc;
      hipLaunchKernelGGL(pb_cells_kernel, dim3((unsigned)fsf_stream_grid(n_pts, 256)), dim3(256), 0, stream, keys, order, n_pts, pts,
                         (int)pts_stride, pts_batch, l.cell_start, l.cell_end, l.sorted);
      PoolBinArgs b{a, order, l.sorted, l.cell_start, l.cell_end, l.hits_full};
      const unsigned wg = (unsigned)((n_rois + 3) / 4);
      hipLaunchKernelGGL(pb_count_kernel, dim3(wg), dim3(256), 0, stream, b);
      rc = exclusive_scan_u32(PoolScanIn{l.roi_total}, PoolScanOut{l.roi_off}, n_rois, l.tile_sums_b, l.total, nullptr, stream, (int64_t)max_inbox_point, true);
      if (rc != FSF_OK) return rc;
      hipLaunchKernelGGL(pb_fill_kernel, dim3(wg), dim3(256), 0, stream, b);
      hipLaunchKernelGGL(pool_count_kernel, dim3(1), dim3(1), 0, stream, l.total, max_all_pts, cdev);
      FSF_LAUNCH_CHECK();
      if (count_host) {
        FSF_READ_BACK(count_host, cdev, sizeof(int64_t), stream);
      }
      return FSF_OK;
    }
    FSF_HIP_TRY(hipMemsetAsync(l.roi_total, 0, sizeof(uint32_t) * n_rois, stream));
    FSF_HIP_TRY(hipMemsetAsync(l.chunk_total, 0, sizeof(uint32_t) * 32, stream));
    const int groups = fsf_cdiv(n_rois, 256);
    for (int g0 = 0, len = 1, chunk = 0; g0 < groups; g0 += len, len = chunk < 30 ? len * 2 : groups, ++chunk) {
      const int ng = g0 + len <= groups ? len : groups - g0;
      a.group0 = g0;
      a.chunk = chunk;
      hipLaunchKernelGGL((pool_pass_kernel<false>), dim3((unsigned)ng, (unsigned)l.pt_tiles), dim3(256), 0, stream, a);
      hipLaunchKernelGGL(pool_prefix_kernel, dim3((unsigned)ng), dim3(256), 0, stream, a, l.pt_tiles);
    }
    a.group0 = 0;
    a.chunk = 0;
    const dim3 grid((unsigned)groups, (unsigned)l.pt_tiles);
    int rc = exclusive_scan_u32(PoolScanIn{l.roi_total}, PoolScanOut{l.roi_off}, n_rois, l.tile_sums, l.total, nullptr, stream, (int64_t)max_inbox_point);
    if (rc != FSF_OK) return rc;
    hipLaunchKernelGGL((pool_pass_kernel<true>), grid, dim3(256), 0, stream, a);
    hipLaunchKernelGGL(pool_count_kernel, dim3(1), dim3(1), 0, stream, l.total, max_all_pts, cdev);
    FSF_LAUNCH_CHECK();
  }
  if (count_host) {
    FSF_READ_BACK(count_host, cdev, sizeof(int64_t), stream);
  }
  return FSF_OK;
}
