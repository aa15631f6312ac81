"""CPU: what tests/test_rulebook_gpu.py stands on.

* The dense referee of tests/rulebook_cases.py (a read of the input cell o * stride - pad + k * dil per output cell and offset) equals
  `oracle.spconv.build_rulebook` (an input proposes an output) on every case whose grid fits a dense array; on the grids of more than
  2^32 cells the oracle equals the dense referee of the same clusters laid into a small grid.
* `paths()` over all cases is exactly the declared tag list, every case reaches the tags it carries, and every tag has a witness
  named here.  The launch rules `paths()` restates are pinned to the source text.
* A numpy model of the device algorithm (hash insert / lookup with linear probing, propose, unique, radix sort on the key's low bits,
  the two tables, pair compaction by 256-row segment) equals the referee on every case, and with each of eight planted defects it
  fails a case named here: the GPU test cannot pass with a kernel that is wrong in one of these ways."""
import os
import re

import numpy as np
import pytest

import rulebook_cases as R
from conftest import ROOT

WITNESS = {
    "propose_rows": "geometry-strided-k3_s2_p1", "propose_rows_lds_over_48k": "geometry-strided-k3_s1_p1",
    "propose_rows_lds_61440": "geometry-strided-k532_s1_p0", "propose_by_pair": "geometry-strided-k442_s1_p0",
    "per_in_8": "geometry-strided-k5_s3_p2_d2", "per_in_27": "geometry-strided-k3_s2_p2_d2",
    "strided_dilation": "geometry-strided-k3_s2_p3_d3", "subm_dilation": "geometry-subm-k3_d2",
    "stride_dilation_share_a_factor": "geometry-strided-k3_s2_p2_d2", "anisotropic": "geometry-strided-k311_s211_p0",
    "stride_3": "geometry-strided-k5_s3_p2_d2", "stride_1_strided": "geometry-strided-k5_s1_p2", "even_kernel": "geometry-strided-k2_s2_p0",
    "kvol_1": "geometry-subm-k1", "no_padding": "geometry-strided-k3_s2_p0", "corner_sites": "geometry-subm-k3",
    "same_site_in_two_batches": "geometry-strided-k3_s2_p1",
    "m_out_zero": "no_output-all", "inverse_dead_rows": "no_output-half",
    "pairs_single_partial_segment": "seg_edges-m255", "pairs_whole_segments": "seg_edges-m256", "pairs_partial_last_segment": "seg_edges-m257",
    "pairs_before_second_trip": "seg_edges-sheet", "pairs_kvol_second_trip": "seg_edges-k7", "pairs_empty_offset": "seg_edges-spread",
    "pairs_dead_row": "no_output-half",
    "cap_1024_load_half": "seg_edges-m512", "cap_2048_smallest": "seg_edges-m513", "hash_wrap_inputs": "hash_wrap-inputs",
    "hash_wrap_outputs": "hash_wrap-outputs",
    "stream_grid_capped": "seg_edges-sheet", "lin_in_over_32_bits": "wide_keys_batch", "lin_out_over_32_bits": "wide_keys_batch",
    "sort_passes_5": "wide_keys_av2", "sort_passes_up_to_4": "geometry-strided-k3_s2_p1",
    "mo_single_row": "mask_order-m1", "mo_odd_m": "mask_order-m63", "mo_even_m": "mask_order-m64", "mo_second_round": "mask_order-sheet",
    "mo_full_row": "mask_order-cube5", "mo_lone_row": "mask_order-lone", "mo_lo_saturates": "mask_order-cube5", "mo_hi_9": "mask_order-cube5",
    "mo_all_parities": "mask_order-cube5"}

# defect -> (case that must fail, entry point whose result differs)
DEFECT_CASES = {
    "bounds_x": ("geometry-strided-k3_s2_p1", "both"), "lin_in_u32": ("wide_keys_av2", "both"), "oz_for_z": ("geometry-strided-k3_s2_p1", "strided"),
    "inverse_ignores_dilation": ("geometry-strided-k3_s2_p2_d2", "strided"), "stride_test_one_axis": ("geometry-strided-k3_s2_p1", "strided"),
    "before_first_256": ("seg_edges-sheet", "pairs"), "probe_no_wrap": ("hash_wrap-inputs", "both"),
    "m_out_zero_unwritten": ("no_output-all", "strided")}


def _same(a, b):
    return all(np.array_equal(x, y) and np.asarray(x).shape == np.asarray(y).shape for x, y in zip(a, b))


def _strided_want(e):
    return e["out_indices"], e["nbr"], e["nbr_inv"]


@pytest.mark.parametrize("name", R.DENSE)
def test_dense_referee_equals_the_oracle(name):
    c, e = R.case(name), R.expected(name)
    idx = c["idx"]
    assert len(set(map(tuple, idx.tolist()))) == idx.shape[0] and (np.diff(R.lin(idx, c["shape"])) > 0).all()
    np.testing.assert_array_equal(e["subm"], R.oracle_subm(idx, c["batch"], c["shape"], c["subm_ksize"], c["subm_dilation"]))
    o_idx, o_nbr, o_inv, o_shape = R.oracle_strided(idx, c["batch"], c["shape"], c["ksize"], c["stride"], c["padding"], c["dilation"])
    assert list(o_shape) == list(e["out_shape"]) and min(o_shape) >= 1
    np.testing.assert_array_equal(e["out_indices"], o_idx.reshape(-1, 4))
    np.testing.assert_array_equal(e["nbr"], o_nbr)
    np.testing.assert_array_equal(e["nbr_inv"], o_inv)
    assert e["nbr"].shape[0] == 0 or (e["nbr"] >= 0).any(1).all()


@pytest.mark.parametrize("name", list(R.WIDE_GRIDS))
def test_wide_key_tables_equal_the_same_clusters_in_a_small_grid(name):
    """Translation invariance: the oracle's tables on the grid of more than 2^32 cells are the dense referee's tables of the same two
    clusters in the interior of a small grid; the output sites are the small grid's shifted by the clusters' translation."""
    c, e = R.case(name), R.expected(name)
    (sshape, sbatch) = R.WIDE_SMALL
    small = R.wide_sites(c["shape"], c["batch"], small=True)
    assert small.shape == c["idx"].shape and 350 <= small.shape[0] <= 500
    shift = c["idx"].astype(np.int64) - small
    n_ghost = len(R.wide_clusters()[1])
    assert len(np.unique(shift, axis=0)) == 2 and (shift[:, 1:] % 2 == 0).all() and n_ghost >= 12
    np.testing.assert_array_equal(e["subm"], R.dense_subm(small, sbatch, sshape, c["subm_ksize"], c["subm_dilation"]))
    s_idx, s_nbr, s_inv, _ = R.dense_strided(small, sbatch, sshape, c["ksize"], c["stride"], c["padding"], c["dilation"])
    np.testing.assert_array_equal(e["nbr"], s_nbr)
    np.testing.assert_array_equal(e["nbr_inv"], s_inv)
    first_in = np.where(s_nbr >= 0, s_nbr, small.shape[0]).min(1)          # an output site moves with the cluster of its inputs
    np.testing.assert_array_equal(e["out_indices"].astype(np.int64) - s_idx, shift[first_in] // np.array([1, 2, 2, 2]))
    # away from every border, in the last batch, and beyond 32 bits in both linearisations
    idx = c["idx"].astype(np.int64)
    assert idx[:, 0].max() == c["batch"] - 1 and (idx[:, 1:] >= 4).all() and (idx[:, 1:] < np.array(c["shape"]) - 4).all()
    assert int(R.lin(idx, c["shape"]).max()) >= 2 ** 32 and int(R.lin(e["out_indices"], e["out_shape"]).max()) >= 2 ** 32
    # every ghost site lies exactly 2^32 cells before an EMPTY in-plane neighbour cell of a main site
    lin = R.lin(idx, c["shape"])
    ghost = lin[np.isin(lin + 2 ** 32, R.lin(idx + np.array([0, 0, 0, 1]), c["shape"])) | np.isin(lin + 2 ** 32, R.lin(idx + np.array([0, 0, 1, 0]), c["shape"]))
                | np.isin(lin + 2 ** 32, R.lin(idx + np.array([0, 0, -1, 1]), c["shape"]))]
    assert len(ghost) == n_ghost and not np.isin(ghost + 2 ** 32, lin).any()
    if name == "wide_keys_av2":
        assert R.sort_passes(c["batch"] * int(np.prod(e["out_shape"]))) == 5


def test_paths_cover_exactly_the_declared_tags_and_every_tag_has_a_witness():
    reached = {name: R.paths(R.case(name)) for name in R.ALL}
    for name in R.ALL:
        assert R.case(name)["tags"] <= reached[name], (name, R.case(name)["tags"] - reached[name])
    assert set().union(*reached.values()) == set(R.FULL_TAGS)
    assert set(WITNESS) == set(R.FULL_TAGS)
    for tag, name in WITNESS.items():
        assert tag in reached[name], (tag, name)
    # the numbers the issue's table names
    assert {g: R.per_in(*[R.STRIDED_GEOMETRIES[g][i] for i in (0, 1, 3)]) for g in R.STRIDED_GEOMETRIES} == {
        "k3_s2_p1": 8, "k3_s2_p011": 8, "k3_s2_p0": 8, "k3_s1_p1": 27, "k3_s2_p2_d2": 27, "k3_s2_p3_d3": 8, "k5_s3_p2_d2": 8,
        "k311_s211_p0": 2, "k133_s122_p011": 4, "k2_s2_p0": 1, "k532_s1_p0": 30, "k442_s1_p0": 32, "k5_s1_p2": 125}
    assert R.rows_kernel_lds(27) == 55296 and R.rows_kernel_lds(30) == 61440 and not R.proposes_by_pair(30) and R.proposes_by_pair(32)
    m = {name: R.case(name)["idx"].shape[0] for name in R.ALL}
    assert all(300 <= m[n] <= 900 for n in R.ALL if n.startswith("geometry")), m
    assert m["seg_edges-sheet"] == 65793 and (m["seg_edges-sheet"] + 255) // 256 == 258 and m["mask_order-sheet"] == 16385
    assert m["seg_edges-k7"] == 300 and int(np.prod(R.case("seg_edges-k7")["subm_ksize"])) == 343
    assert max(m.values()) == 65793 and sorted(m.values())[-2] == 16385
    # the LDS list of the rows kernel really fills: at stride 1 a workgroup's 256 inputs are first to propose more sites than it has threads
    e = R.expected("geometry-strided-k3_s1_p1")
    assert e["nbr"].shape[0] > 2 * m["geometry-strided-k3_s1_p1"]
    # the mask-order key with both saturations reached: all nine below (lo = 7), all nine above (hi = 9, never 15)
    key, mid, lo, hi = R.mask_order_key(R.expected("mask_order-cube5")["nbr27"])
    assert ((mid == 511) & (lo == 7) & (hi == 9)).sum() == 27 and int(hi.max()) == 9
    lone = R.expected("mask_order-lone")["nbr27"]
    assert ((lone >= 0).sum(1) == 1).all() and (R.mask_order_key(lone)[1] == 16).all()
    spread = R.expected("seg_edges-spread")["subm"]
    assert (spread[:, 13] == np.arange(spread.shape[0])).all() and (np.delete(spread, 13, 1) < 0).all()


def test_hash_wrap_is_forced():
    """More keys have their home in the last three slots of the 1024-slot table than there are slots there, and the first nine slots
    have tenants of their own: the chain wraps through (slot + 1) & mask and displaces them in turn."""
    for name, cells, cap in (("hash_wrap-inputs", R.lin(R.case("hash_wrap-inputs")["idx"], R.case("hash_wrap-inputs")["shape"]), 1024),
                             ("hash_wrap-outputs", R.lin(R.expected("hash_wrap-outputs")["out_indices"], R.expected("hash_wrap-outputs")["out_shape"]),
                              R.pow2_at_least(2 * R.case("hash_wrap-outputs")["idx"].shape[0] * 8))):
        assert cap == 1024 and len(cells) <= 512
        home = (R.hash_mix(cells) & np.uint64(cap - 1)).astype(np.int64)
        assert (home >= cap - 3).sum() >= 12 and all((home == s).sum() >= 1 for s in range(9)), name
        t = R.HashTable(cap)
        t.insert(cells, np.arange(len(cells)))
        moved = np.array([int(np.nonzero(t.keys == np.uint64(k))[0][0]) for k in cells]) != home
        assert moved[home >= cap - 3].sum() >= 9 and moved[home < 9].any(), name    # tenants of the last slots live in slots 0, 1, 2, ...
        np.testing.assert_array_equal(t.lookup(cells), np.arange(len(cells)))
    c = R.case("hash_wrap-outputs")
    assert R.expected("hash_wrap-outputs")["nbr"].shape[0] == c["idx"].shape[0]      # one output site per input


def test_hash_mix_is_the_kernels():
    # splitmix / murmur3 finaliser: fmix64(1) and fmix64(2^32) computed with Python integers
    def ref(k):
        k ^= k >> 33
        k = k * 0xff51afd7ed558ccd % 2 ** 64
        k ^= k >> 33
        k = k * 0xc4ceb9fe1a85ec53 % 2 ** 64
        return k ^ (k >> 33)

    keys = [0, 1, 2 ** 32, 2 ** 37 + 12345, 2 ** 63 + 7]
    assert [int(v) for v in R.hash_mix(np.array(keys, np.uint64))] == [ref(k) for k in keys]


def _src(*parts):
    return open(os.path.join(ROOT, "fullysparsefusion_amd", *parts)).read()


def test_constants_and_rules_equal_the_kernel_source():
    rb, common, radix, ops = _src("csrc", "rulebook.hip"), _src("csrc", "common.h"), _src("csrc", "radix_sort.hip"), _src("hip_ops.py")
    assert int(re.search(r"constexpr int RBP_SEG = (\d+);", rb).group(1)) == R.RBP_SEG
    assert rb.count("__launch_bounds__(256)") == rb.count("__global__") and R.BLOCK == 256
    grid = common[common.index("static inline int fsf_stream_grid("):][:300]
    assert "if (g > %d) g = %d;" % (R.STREAM_GRID_MAX, R.STREAM_GRID_MAX) in grid and "(work_items + block - 1) / block" in grid
    p2 = rb[rb.index("static uint64_t pow2_at_least("):][:200]
    assert "uint64_t p = %d;" % R.HASH_CAP_FLOOR in p2 and "while (p < v) p <<= 1;" in p2
    for line in ("const int64_t cap = (int64_t)pow2_at_least((uint64_t)m * 2);", "const int64_t in_cap = (int64_t)pow2_at_least((uint64_t)m * 2);",
                 "const int64_t set_cap = (int64_t)pow2_at_least((uint64_t)(m * per_in) * 2);",
                 "const int pz_ = g.sz / gcd(g.sz, g.dz), py_ = g.sy / gcd(g.sy, g.dy), px_ = g.sx / gcd(g.sx, g.dx);",
                 "const int64_t per_in = (int64_t)((g.kz + pz_ - 1) / pz_) * ((g.ky + py_ - 1) / py_) * ((g.kx + px_ - 1) / px_);",
                 "256 * per_in * 8 + 8 > 64 * 1024", "(size_t)256 * per_in * 8, stream", "bit_width64(total_cells - 1)",
                 "const uint64_t total_cells = (uint64_t)g.B * g.OZ * g.OY * g.OX;",
                 "slot = (slot + 1) & mask;", "for (int s = threadIdx.x; s < seg; s += 256)", "for (int k = threadIdx.x; k < kvol; k += 256)",
                 "const int64_t halves = ((int64_t)gridDim.x * blockDim.x) >> 5;", "fsf_stream_grid(m * 32, 256)",
                 "const uint32_t lo = min(__popc(mask & 511u), 7), hi = min(__popc(mask >> 18), 15);",
                 "if (ksize[j] % 2 == 0) return FSF_ERR_UNSUPPORTED;", "if (g->OZ < 1 || g->OY < 1 || g->OX < 1) return FSF_ERR_INVALID_ARG;"):
        assert line in rb, line
    assert rb.count("slot = (slot + 1) & mask;") == 3 and R.LDS_NO_ATTRIBUTE == 64 * 1024
    assert "const int passes_all = (key_bits + 7) / 8;" in radix and "p * 8," in radix and R.RADIX_BITS == 8
    assert "nbr_inv = torch.empty((m, kvol), dtype=torch.int32, device=dev) if want_inverse else None" in ops
    assert "cap = max(1, min(m * kvol, cells))" in ops
    # the rules in numbers
    assert [R.pow2_at_least(2 * m) for m in (1, 511, 512, 513, 1024, 1025)] == [1024, 1024, 1024, 2048, 2048, 4096]
    assert [R.sort_passes(v) for v in (1, 2, 256, 257, 2 ** 32, 2 ** 32 + 1, 2 * 21 * 20000 * 20000)] == [0, 1, 1, 2, 4, 5, 5]
    assert R.stream_grid(1) == 1 and R.stream_grid(2048 * 256 + 1) == 2048 and R.stream_grid(16385 * 32) * 256 // 32 == 16384


# ---- the model of the device algorithm ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", R.ALL)
def test_model_of_the_device_algorithm_equals_the_referee(name):
    c, e = R.case(name), R.expected(name)
    np.testing.assert_array_equal(R.model_subm(c), e["subm"])
    out_idx, nbr, nbr_inv, oshape = R.model_strided(c)
    assert list(oshape) == list(e["out_shape"])
    np.testing.assert_array_equal(out_idx, e["out_indices"].reshape(-1, 4))
    np.testing.assert_array_equal(nbr, e["nbr"])
    np.testing.assert_array_equal(nbr_inv, e["nbr_inv"])
    for table in (e["subm"], e["nbr"], e["nbr_inv"]):
        pairs, num = R.model_pairs(table)
        for k, (i_r, o_r) in enumerate(R.table_pairs(table)):
            assert num[k] == len(i_r)
            np.testing.assert_array_equal(pairs[k, 0, :num[k]], i_r)
            np.testing.assert_array_equal(pairs[k, 1, :num[k]], o_r)
            assert (pairs[k, :, num[k]:] == -1).all()


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_each_planted_defect_fails_its_case(defect):
    name, where = DEFECT_CASES[defect]
    c, e = R.case(name), R.expected(name)
    if where == "pairs":
        pairs, num = R.model_pairs(e["subm"], defect)
        good = R.model_pairs(e["subm"])
        assert not (np.array_equal(pairs, good[0]) and np.array_equal(num, good[1]))
        assert (e["subm"].shape[0] + R.RBP_SEG - 1) // R.RBP_SEG - 1 > R.BLOCK
        return
    subm_ok = np.array_equal(R.model_subm(c, defect), e["subm"])
    got = R.model_strided(c, defect)
    strided_ok = _same(got[:3], _strided_want(e))
    assert not strided_ok, defect
    if where == "both":
        assert not subm_ok, defect
    if defect == "m_out_zero_unwritten":
        assert got[1].shape[0] == 0 and (got[2] == R.POISON).all() and (e["nbr_inv"] == -1).all()
    if defect == "probe_no_wrap":
        c2, e2 = R.case("hash_wrap-outputs"), R.expected("hash_wrap-outputs")
        assert not _same(R.model_strided(c2, defect)[:3], _strided_want(e2))


def test_defect_list_is_the_one_the_cases_were_built_against():
    assert set(DEFECT_CASES) == set(R.DEFECTS) and len(R.DEFECTS) == 8
