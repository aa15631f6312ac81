"""CPU: what the crafted weight-gradient cases of tests/wgrad_cases.py (run on the device by tests/test_wgrad_gpu.py) stand on.

* Every path tag is reached by a case, and each of the four kernels meets both sides of the range split, a dead split, an empty offset
  and a last stage that cuts a 4-pair micro-tile.
* A numpy model of the two launches of csrc/spconv_bwd.hip — splits of `range` pairs, 32-pair stages whose index loads are clamped to
  p_end - 1 and whose rows past p_end are zero-filled, one partial slice per live split in a workspace that still holds an older call's
  sums, the fold over the `live` slices in the kernel's slice / unroll order, the zero write for an empty offset — equals the referee on
  every case, and with each of nine planted defects it fails a case this module names.  The model forms a stage's product in float64:
  in these families every partial sum is exact, so the order inside a stage is no part of what is modelled.
* The workspace the model starts from holds STALE everywhere (the device test fills it by a real call with every list full); the result
  it writes into starts as NaN, so a slice nobody writes is seen."""
import time

import numpy as np
import pytest

import product_budget as P
import wgrad_cases as W

SPENT = [0.0]  # seconds inside this module's tests (the cases are built inside them)
STALE = np.float32(3.0)
DEFECTS = ("no_zero_fill", "fold_all_splits", "empty_unwritten", "tail_u_lt_2", "no_main_loop", "pin_pout_swapped", "tiles_a_for_tiles_b",
           "stale_stage_indices", "p_end_unclamped")


@pytest.fixture(autouse=True)
def _stopwatch():
    t0 = time.perf_counter()
    yield
    SPENT[0] += time.perf_counter() - t0


def model(c, d, defect=None):
    """f32 [kvol, cin, cout] of case `c` with data `d` = W.case(name)."""
    ta, tb, tiles_a, tiles_b, nsplit, rng = W.plan(c)
    feat, gout, pairs = d["feat"].astype(np.float64), d["gout"].astype(np.float64), d["pairs"]
    gw = np.full((c.kvol, c.cin, c.cout), np.nan, np.float32)
    part = np.full((c.kvol, nsplit, c.cin, c.cout), STALE, np.float32) if nsplit > 1 else None
    last_slot = c.cap - 1
    # ---- launch 1: grid (split, offset, channel tile)
    for k, n in enumerate(c.counts):
        for split in range(nsplit):
            p_begin = split * rng
            if p_begin >= n:
                continue
            p_end = p_begin + rng if defect == "p_end_unclamped" else min(n, p_begin + rng)
            nst = W.cdiv(p_end - p_begin, W.BW_RT)
            p = p_begin + np.arange(nst * W.BW_RT)
            valid = p < p_end
            slot = p.copy()
            if defect == "stale_stage_indices":  # from the third stage on, the registers hold the indices of the stage after it
                slot[2 * W.BW_RT:] += W.BW_RT
            slot = np.minimum(np.minimum(slot, p_end - 1), last_slot)  # (the second bound keeps the MODEL of defect 9 in range)
            if pairs is None:
                ii = oo = slot
            else:
                ii, oo = pairs[k, 0, slot], pairs[k, 1, slot]
                if defect == "pin_pout_swapped":
                    ii, oo = np.minimum(oo, c.m_in - 1), np.minimum(ii, c.m_out - 1)
            keep = np.ones_like(valid) if defect == "no_zero_fill" else valid
            a, b = feat[ii] * keep[:, None], gout[oo] * keep[:, None]
            dst = part[k, split] if nsplit > 1 else gw[k]
            for z in range(tiles_a * tiles_b):
                div = tiles_a if defect == "tiles_a_for_tiles_b" else tiles_b
                a0, b0 = (z // div) * ta, (z % div) * tb
                if a0 < c.cin and b0 < c.cout:
                    dst[a0:a0 + ta, b0:b0 + tb] = a[:, a0:a0 + ta].T @ b[:, b0:b0 + tb]
    # ---- launch 2: the fold
    for k, n in enumerate(c.counts):
        live = nsplit if defect == "fold_all_splits" else W.cdiv(n, rng)
        if nsplit > 1:
            red = []
            for sl in range(16):
                acc = [np.zeros((c.cin, c.cout), np.float32) for _ in range(4)]
                i = sl
                while i + 48 < live and defect != "no_main_loop":
                    for u in range(4):
                        acc[u] += part[k, i + 16 * u]
                    i += 64
                for u in range(2 if defect == "tail_u_lt_2" else 3):
                    if i + 16 * u < live:
                        acc[u] += part[k, i + 16 * u]
                red.append((acc[0] + acc[1]) + (acc[2] + acc[3]))
            s = np.zeros((c.cin, c.cout), np.float32)
            for r in red:
                s += r
            gw[k] = s
        elif live == 0 and defect != "empty_unwritten":
            gw[k] = 0.0
    return gw


def _equal(got, want):
    return np.array_equal(got.view(np.uint32), want.view(np.uint32))


# defect -> a case it must fail on (and why)
CAUGHT_ON = {
    "no_zero_fill": "A-68x68-shuffled-ints",             # num = 1, 3, 5, 31 ...: the clamped last pair is added 31, 29, ... more times
    "fold_all_splits": "B-68x68-shuffled-ints",          # dead splits' slices hold an older call's sums
    "empty_unwritten": "A-64x64-ascending-ints",         # num[0] = 0 under nsplit = 1
    "tail_u_lt_2": "B-20x132-shuffled-ints",             # live = 48: slices 32 .. 47 are the tail's third
    "no_main_loop": "B-132x20-ascending-ints",           # live = 49: slice 48 is only in the main loop's reach
    "pin_pout_swapped": "A-132x20-mixed-ints",           # m_in != m_out, different draws on the two sides
    "tiles_a_for_tiles_b": "A-132x20-ascending-ints",    # tiles_a = 2, tiles_b = 1: the second `a` tile is never written
    "stale_stage_indices": "A-128x128-shuffled-ints",    # num = 95, 97, 255, 256: three stages and more
    "p_end_unclamped": "A-4x4-one_row-ints",             # slots past num[k] name the poison row
}
# the one-hot families catch the defects that move a value too
ALSO_CAUGHT_ON = {"no_zero_fill": "H-68x68-ascending-one_hot", "pin_pout_swapped": "H-132x260-ascending-one_hot_t",
                  "tiles_a_for_tiles_b": "H-132x260-one_row-one_hot",
                  "fold_all_splits": "C-132x260-mixed-ints", "p_end_unclamped": "B-64x64-one_row-ints"}


@pytest.mark.parametrize("name", W.NAMES)
def test_model_equals_the_referee(name):
    d = W.case(name)
    c = d["case"]
    assert c.family in W.EXACT_FAMILIES
    W.check_exact(name, model(c, d), d["want"])
    # the poison row: last of both operands, 2^20 everywhere, named by every dead slot and by no live one
    if c.num is not None:
        assert (d["feat"][-1] == W.POISON).all() and (d["gout"][-1] == W.POISON).all()
        assert d["pairs"].shape == (c.kvol, 2, c.cap) and d["pairs"].min() >= 0
        for k, n in enumerate(c.num):
            assert (d["pairs"][k, 0, n:] == c.m_in - 1).all() and (d["pairs"][k, 1, n:] == c.m_out - 1).all()
            assert (d["pairs"][k, 0, :n] < c.m_in - 1).all() and (d["pairs"][k, 1, :n] < c.m_out - 1).all()
    else:
        assert d["feat"].shape[0] == d["gout"].shape[0] == c.cap and np.abs(d["feat"]).max() <= 8
    assert np.abs(d["want"]).max(initial=0.0) < W.POISON


@pytest.mark.parametrize("defect", DEFECTS)
def test_every_planted_defect_fails_its_named_case(defect):
    for name in (CAUGHT_ON[defect], ALSO_CAUGHT_ON.get(defect)):
        if name is not None:
            d = W.case(name)
            assert _equal(model(d["case"], d), d["want"])
            assert not _equal(model(d["case"], d, defect), d["want"]), (defect, name)


def test_patterns_are_what_they_are_called():
    for name in W.NAMES:
        c = W.SPECS[name]
        if c.num is None:
            continue
        d = W.case(name)
        hot = {"one_hot": 1, "one_hot_t": 0}.get(c.family)
        for k, n in enumerate(c.num):
            i, o = d["pairs"][k, 0, :n], d["pairs"][k, 1, :n]
            if c.pattern == "ascending":
                assert (np.diff(i) > 0).all() and (np.diff(o) > 0).all()
            if c.pattern == "one_row":
                assert len(set((o if hot == 0 else i).tolist())) <= 1
            if hot is not None:  # the hot channels of an offset's pairs all differ, every element is one product
                rows, op, ch = (i, d["feat"], c.cin) if hot == 0 else (o, d["gout"], c.cout)
                assert len(set((rows % ch).tolist())) == n and (np.count_nonzero(op[rows], axis=1) == 1).all()
                assert n <= min(c.cin, c.cout)
        if c.pattern == "mixed":
            assert c.m_in != c.m_out
        if hot is not None:
            full, one = (d["gout"], d["feat"]) if hot == 0 else (d["feat"], d["gout"])
            mant = np.frexp(np.abs(one[:-1][one[:-1] != 0]))[0]
            assert (mant == 0.5).all()                                              # +-2^t
            assert (full[:-1].view(np.uint32) & 0xFF).astype(bool).mean() > 0.9     # the lo piece is live
            assert sorted(c.num) == list(c.num) and c.num[-1] == min(65, c.cin, c.cout)
    shuffled = W.case("A-68x68-shuffled-ints")["pairs"][14, 0]
    assert (np.diff(shuffled) < 0).any() and len(set(shuffled.tolist())) == 256


def test_every_tag_is_reached():
    reached = {}
    for name in W.NAMES:
        for t in W.paths(W.SPECS[name]):
            reached.setdefault(t, name)
    assert W.FULL_TAGS <= set(reached), sorted(W.FULL_TAGS - set(reached))
    # the lists: the plans the cases were chosen for
    for name in W.find("A"):
        assert W.plan(W.SPECS[name])[4:] == (1, 256), name
    for name in W.find("B"):
        assert W.plan(W.SPECS[name])[4:] == (130, 256) and W.live_splits(W.SPECS[name]) == [0, 1, 1, 2, 16, 17, 48, 49, 64, 65, 112, 113, 130]
    assert len(W.find("B")) == 8 and {(W.SPECS[n].cin, W.SPECS[n].cout) for n in W.find("B")} == set(W.KERNEL_SHAPE.values())
    for name in W.find("C"):
        c = W.SPECS[name]
        assert W.plan(c) == (128, 128, 2, 3, 9, 256) and set(W.live_splits(c)) == set(range(10))
        assert {"fold_grid_stride", "tiles_a_ne_tiles_b", "multi_tile_a", "multi_tile_b", "nsplit_gt1", "dead_split"} <= W.paths(c)
    assert {(W.SPECS[n].cin, W.SPECS[n].cout) for n in W.find("A")} == set(W.SHAPES) and len(W.find("A")) == 28
    assert [W.plan(W.SPECS[n])[4] for n in W.find(shape=(68, 68), pattern="identity")] == [1, 1, 1, 1, 2, 9]
    assert sum(W.LIST_B[1]) == 156678 and max(W.LIST_B[1]) == W.LIST_B[0]
    # tags that name one decision each
    assert "min_width" in W.paths(W.SPECS["A-4x4-mixed-ints"]) and "full_tile" in W.paths(W.SPECS["A-128x128-mixed-ints"])
    assert {"partial_tile_a", "partial_tile_b", "clamped_quad"} <= W.paths(W.SPECS["A-68x68-mixed-ints"])
    assert "last_split_one_pair" in W.paths(W.SPECS["B-64x64-ascending-ints"])


def test_every_kernel_meets_both_sides_of_the_split_and_a_cut_micro_tile():
    for kernel, shape in W.KERNEL_SHAPE.items():
        tags = set()
        for name in W.find(shape=shape):
            assert W.kernel_tag(W.SPECS[name]) == kernel
            tags |= W.paths(W.SPECS[name])
        assert {"nsplit_1", "nsplit_gt1", "dead_split", "empty_offset_nsplit1", "empty_offset_nsplit_gt1", "num_eq_cap", "stages_1", "stages_2",
                "stages_3plus", "full_last_stage", "last_split_one_pair"} <= tags, kernel
        assert {"rem_1", "rem_3", "rem_5", "rem_31", "rem_4"} <= tags, kernel
        assert {"live_%d" % v for v in W.LIVE_EDGES} <= tags, kernel
    assert {W.kernel_tag(W.SPECS[n]) for n in W.NAMES} == set(W.KERNEL_TAGS)
    assert {P.wgrad_kernel(*s) for s in ((4, 4), (64, 64), (20, 132), (132, 20))} == {"K10"}
    assert {P.wgrad_kernel(*s) for s in ((68, 68), (128, 128), (132, 260))} == {"K10p"}


def test_stale_workspace_cases_and_their_filling_call():
    names = [n for n in W.NAMES if W.needs_stale_workspace(W.SPECS[n])]
    assert sorted(names) == sorted(W.find("B") + W.find("C"))
    c = W.SPECS[names[0]]
    f1, g1 = W.operands(c)
    f2, g2 = W.operands(c, key=7)
    assert f1.shape == f2.shape and (f1[:-1] != f2[:-1]).mean() > 0.5 and (g1[:-1] != g2[:-1]).mean() > 0.5


def test_module_runs_in_under_a_minute():
    """(Collected last: the stopwatch has summed every test above when the module is run whole.)"""
    assert SPENT[0] < 60.0, SPENT[0]
