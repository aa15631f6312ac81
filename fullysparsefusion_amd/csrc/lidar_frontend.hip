// K30: the LiDAR-query branch's clustering front end as ONE native call (round 6; VERDICT r5 next-1: "stage-level native entry points
// that sequence their kernels from C++ on the caller's stream").
//
// SingleStageFSD.group_sample (detectors/single_stage_fsd.py:802-865) + ClusterAssigner.forward (:903-982) + update_sample_results_by_mask
// (:867-890) + combine_classes (:892-901) + the cluster centroids of SingleStageFSD.extract_feat (:458-474), for ALL class groups of ONE
// sample, were eleven C-ABI calls issued from Python with four host waits between them (pair count, voxel-key count, survivor counts,
// cluster count): after every wait the interpreter took 30-110 us to reach the next launch — on the frame's critical path, and under a
// lock it shares with the camera-query branch's host thread.  Here the same eleven entry points are called back to back from C++: the
// waits are still there (each count sizes what follows) but what follows is issued microseconds later, and the calling thread holds no
// interpreter lock while it waits.  Same kernels, same order, same arguments: results are bit-identical to the Python sequence
// (tests/test_lidar_frontend_gpu.py).
//
// Memory: the caller hands over ONE arena (fsf_lidar_cluster_frontend_arena_bytes(m, ng, point_cols): the worst case, every (group, point)
// pair surviving); intermediates and results are bump-allocated inside it in the order below, and the results' byte offsets + row counts
// come back in `out` (host i64 [FSF_LCF_OUT_WORDS]).  Nothing is allocated or freed here.  The size is computed by running the entry's
// own stage layouts (LcfPairs ... LcfCentroids) on a measuring arena with every count at its worst case.
#include "common.h"

namespace {

// One layout per stage: a stage ends where the device tells the host a count (P pairs, K voxel keys, K' kept keys and V kept pairs,
// C clusters) that sizes the next one.  The entry point runs them in this order with the counts it reads back, the size query with
// cap = max(m, 1) * ng for every count.  The scratch of a nested entry point is one slice of that entry's own size query.
struct LcfWs {
  int64_t bytes;
  void* p;
  LcfWs(FsfArena& a, int64_t n) : bytes(n), p(a.take_bytes(n)) {}
};
// the outputs and scratch of one fsf_unique_rows over n rows of k columns
struct LcfUnique {
  int64_t *rows, *inv, *cnt;
  int32_t *order, *offs;
  int64_t* m_dev;
  LcfWs ws;
  LcfUnique(FsfArena& a, int64_t n, int32_t k)
      : rows(a.take<int64_t>(n * k)), inv(a.take<int64_t>(n)), cnt(a.take<int64_t>(n)), order(a.take<int32_t>(n)),
        offs(a.take<int32_t>(n + 1)), m_dev(a.take<int64_t>(1)), ws(a, fsf_unique_rows_workspace_bytes(n, k)) {}
};
// (group, point) pairs of the grouped sampling (:826-838)
struct LcfPairs {
  int64_t *g_ids, *p_ids;
  LcfWs ws;
  LcfPairs(FsfArena& a, int64_t m, int32_t ng)
      : g_ids(a.take<int64_t>(m * ng)), p_ids(a.take<int64_t>(m * ng)), ws(a, fsf_group_pairs_workspace_bytes(m, ng)) {}
};
// vote centres and cluster-voxel keys of every pair (:840-865, :945-950); one unique over the keys of all groups (:31-35 per group upstream)
struct LcfVotes {
  float* centers;
  int64_t *keys, *b_pts;
  LcfUnique uq;
  LcfVotes(FsfArena& a, int64_t P) : centers(a.take<float>(P * 3)), keys(a.take<int64_t>(P * 4)), b_pts(a.take<int64_t>(P)), uq(a, P, 4) {}
};
// the density filter (:951-956): surviving keys / pairs
struct LcfSurvival {
  int64_t* k_idx;
  int32_t* k_group;
  int64_t *v_idx, *vox_inv;
  LcfWs ws;
  LcfSurvival(FsfArena& a, int64_t K, int64_t P)
      : k_idx(a.take<int64_t>(K)), k_group(a.take<int32_t>(K)), v_idx(a.take<int64_t>(P)), vox_inv(a.take<int64_t>(P)),
        ws(a, fsf_cluster_key_survival_workspace_bytes(K, P)) {}
};
// voxel centroids of the votes (every key's, then the survivors' rows), the survivors of the per-pair tensors, connected components of
// the kept voxels per group (:45-82), cluster ids of the pairs (:971-977), the pairs' point rows, and the SIR stack's one unique over
// (group, sample, cluster id) (models/backbones/sir.py:68)
struct LcfClusters {
  float *all_means, *vox_centers;
  int64_t *g_out, *p_out, *b_out;
  float* centers_out;
  int32_t* labels;
  LcfWs cc_ws, id_ws;
  int64_t* pci;
  float* pts_out;
  LcfUnique uq;
  LcfClusters(FsfArena& a, int64_t K, int64_t Kk, int64_t V, int32_t point_cols)
      : all_means(a.take<float>(K * 3)), vox_centers(a.take<float>(Kk * 3)), g_out(a.take<int64_t>(V)), p_out(a.take<int64_t>(V)),
        b_out(a.take<int64_t>(V)), centers_out(a.take<float>(V * 3)), labels(a.take<int32_t>(Kk)),
        cc_ws(a, fsf_connected_components_workspace_bytes(Kk)), id_ws(a, 256), pci(a.take<int64_t>(V * 3)),
        pts_out(a.take<float>(V * (int64_t)point_cols)), uq(a, V, 3) {}
};
// the cluster centroids (:458-474)
struct LcfCentroids {
  float* cluster_xyz;
  LcfWs ws;
  LcfCentroids(FsfArena& a, int64_t V, int64_t C) : cluster_xyz(a.take<float>(C * 3)), ws(a, fsf_segment_reduce_workspace_bytes(V, C, 3)) {}
};

}  // namespace

extern "C" int64_t fsf_lidar_cluster_frontend_arena_bytes(int64_t m, int32_t ng, int32_t point_cols) {
  if (m < 0 || ng < 1 || point_cols < 3) return 0;
  const int64_t m1 = m > 0 ? m : 1, cap = m1 * ng;  // every pair survives every filter: P = K = K' = V = C = cap
  FsfArena a = FsfArena::measure();
  LcfPairs(a, m1, ng);
  LcfVotes(a, cap);
  LcfSurvival(a, cap, cap);
  LcfClusters(a, cap, cap, cap, point_cols);
  LcfCentroids(a, cap, cap);
  return a.used;
}

// out (host): see FSF_LCF_* in include/fsf_hip.h
extern "C" int fsf_lidar_cluster_frontend(const float* scores, int64_t m, int32_t num_classes, int64_t score_stride, const float* thresh,
                                          int32_t ng, const uint32_t* group_class_masks, const float* logits, int32_t logit_stride,
                                          const float* offsets, int32_t offset_stride, const float* points, int32_t point_stride,
                                          int32_t point_cols, const int64_t* batch_idx, const float* group_voxel_size,
                                          const float range_min[3], const int64_t key_min[4], const int64_t key_max[4], int64_t min_points,
                                          const float* dist_table, void* arena, int64_t arena_bytes, int64_t* out, void* stream) {
  if (m < 1 || ng < 1 || ng > 32 || !scores || !thresh || !group_class_masks || !logits || !offsets || !points || !group_voxel_size ||
      !range_min || !key_min || !key_max || !dist_table || !arena || !out || point_cols < 3 || point_stride < point_cols)
    return FSF_ERR_INVALID_ARG;
  // (up front, against the worst case: the stages below launch before the last of them takes its slices)
  if (arena_bytes < fsf_lidar_cluster_frontend_arena_bytes(m, ng, point_cols) || ((uintptr_t)arena & 255)) return FSF_ERR_WORKSPACE;
  for (int i = 0; i < FSF_LCF_OUT_WORDS; ++i) out[i] = 0;
  FsfArena a(arena, arena_bytes);
  const int64_t cap = m * ng;
  int rc;

  const LcfPairs pr(a, m, ng);
  int64_t P = 0;
  rc = fsf_group_pairs(scores, m, ng, score_stride, thresh, 1, group_class_masks, num_classes, pr.g_ids, pr.p_ids, cap, &P, pr.ws.p, pr.ws.bytes,
                       stream);
  if (rc != FSF_OK) return rc;
  if (P < 1) return FSF_ERR_INVALID_ARG;  // (keep_one leaves at least one pair per group)

  const LcfVotes vt(a, P);
  rc = fsf_vote_centers_keys(logits, logit_stride, offsets, offset_stride, points, point_stride, batch_idx, pr.g_ids, pr.p_ids, P, num_classes,
                             ng, group_class_masks, group_voxel_size, range_min, 1, vt.centers, vt.keys, vt.b_pts, stream);
  if (rc != FSF_OK) return rc;
  const LcfUnique& u1 = vt.uq;
  int64_t K = 0;
  rc = fsf_unique_rows(vt.keys, P, 4, key_min, key_max, u1.rows, u1.inv, u1.cnt, u1.order, u1.offs, u1.m_dev, &K, u1.ws.p, u1.ws.bytes, stream);
  if (rc == FSF_ERR_KEY_RANGE)  // a vote outside the caller's bounds: the data-dependent range pass (as sst_ops.unique_with_plan does)
    rc = fsf_unique_rows(vt.keys, P, 4, nullptr, nullptr, u1.rows, u1.inv, u1.cnt, u1.order, u1.offs, u1.m_dev, &K, u1.ws.p, u1.ws.bytes, stream);
  if (rc != FSF_OK) return rc;

  const LcfSurvival sv(a, K, P);
  int64_t counts[2] = {0, 0};
  rc = fsf_cluster_key_survival(u1.rows, 4, u1.cnt, K, u1.inv, P, 1, min_points, ng, sv.k_idx, sv.k_group, sv.v_idx, sv.vox_inv, counts, sv.ws.p,
                                sv.ws.bytes, stream);
  if (rc != FSF_OK) return rc;
  const int64_t Kk = counts[0], V = counts[1];

  const LcfClusters cl(a, K, Kk, V, point_cols);
  {
    const float* fp[1] = {vt.centers};
    const int64_t st[1] = {3};
    const int32_t cs[1] = {3};
    float* op[1] = {cl.all_means};
    rc = fsf_segment_reduce_short(fp, st, cs, 1, P, u1.order, u1.offs, K, 1 /* mean */, op, nullptr, stream);
    if (rc != FSF_OK) return rc;
  }
  rc = fsf_compact_pairs(cl.all_means, 3, sv.k_idx, Kk, cl.vox_centers, pr.g_ids, pr.p_ids, vt.b_pts, vt.centers, sv.v_idx, V, cl.g_out, cl.p_out,
                         cl.b_out, cl.centers_out, stream);
  if (rc != FSF_OK) return rc;
  rc = fsf_connected_components_grouped(cl.vox_centers, Kk, 3, sv.k_group, dist_table, ng, cl.labels, nullptr, cl.cc_ws.p, cl.cc_ws.bytes, stream);
  if (rc != FSF_OK) return rc;
  rc = fsf_cluster_point_ids(cl.labels, sv.k_group, Kk, sv.vox_inv, cl.g_out, cl.b_out, V, ng, cl.pci, cl.id_ws.p, cl.id_ws.bytes, stream);
  if (rc != FSF_OK) return rc;
  rc = fsf_gather_rows_strided(points, point_stride, m, point_cols, cl.p_out, V, cl.pts_out, point_cols, stream);
  if (rc != FSF_OK) return rc;
  const LcfUnique& u2 = cl.uq;
  const int64_t c_min[3] = {0, 0, 0}, c_max[3] = {ng - 1, 0, Kk > 0 ? Kk - 1 : 0};
  int64_t C = 0;
  rc = fsf_unique_rows(cl.pci, V, 3, c_min, c_max, u2.rows, u2.inv, u2.cnt, u2.order, u2.offs, u2.m_dev, &C, u2.ws.p, u2.ws.bytes, stream);
  if (rc == FSF_ERR_KEY_RANGE)
    rc = fsf_unique_rows(cl.pci, V, 3, nullptr, nullptr, u2.rows, u2.inv, u2.cnt, u2.order, u2.offs, u2.m_dev, &C, u2.ws.p, u2.ws.bytes, stream);
  if (rc != FSF_OK) return rc;

  const LcfCentroids ce(a, V, C);
  if (!a.ok()) return FSF_ERR_WORKSPACE;
  rc = fsf_segment_reduce(cl.centers_out, 3, V, 3, u2.order, u2.inv, u2.offs, C, 1 /* mean */, ce.cluster_xyz, nullptr, ce.ws.p, ce.ws.bytes, stream);
  if (rc != FSF_OK) return rc;

  auto off = [&](const void* p) { return (int64_t)((const char*)p - (const char*)arena); };  // (every slice was taken: a.ok())
  out[FSF_LCF_PAIRS] = P; out[FSF_LCF_KEYS] = K; out[FSF_LCF_KEPT_KEYS] = Kk; out[FSF_LCF_ROWS] = V; out[FSF_LCF_CLUSTERS] = C;
  out[FSF_LCF_OFF_P_IDS] = off(cl.p_out); out[FSF_LCF_OFF_CENTERS] = off(cl.centers_out); out[FSF_LCF_OFF_CLUSTER_INDS] = off(cl.pci);
  out[FSF_LCF_OFF_POINTS] = off(cl.pts_out); out[FSF_LCF_OFF_NEW_COORS] = off(u2.rows); out[FSF_LCF_OFF_INV] = off(u2.inv);
  out[FSF_LCF_OFF_CNT] = off(u2.cnt); out[FSF_LCF_OFF_ORDER] = off(u2.order); out[FSF_LCF_OFF_SEG_OFFSETS] = off(u2.offs);
  out[FSF_LCF_OFF_CLUSTER_XYZ] = off(ce.cluster_xyz);
  return FSF_OK;
}
