"""The parts of the second-sweep and family-sweep tests that need no GPU: every case of
tests/test_gpu_second_sweep.py and tests/test_gpu_family_sweep.py is generated on the host,
each second-sweep shape is shown to cross its threshold with the predicate the GPU test calls,
the sweep seeds are shown to reach every family, element type, storage kind, batch and length
law, and the AdaGrad reference vectorised across columns is shown to equal
tests/test_gpu_adagrad.py's per-occurrence ``ref_step`` bit for bit."""
import numpy as np
import pytest

import sweep_cases as sc


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


# --- the thresholds restated on the host are the launch code's --------------------------------

def test_chunk_constant_is_the_library_header():
    from embtab import _lib

    assert sc.CHUNK == _lib.ET_SGD_CHUNK == 256


def test_threshold_arithmetic():
    assert sc.BAG_IDS_BAGS == 262144 and sc.APPLY_COLUMNS == 65536
    assert [sc.sgd_grid(n) for n in (1, 524288, 524289, 2107400, 1 << 30)] == [
        256, 256, 257, 1030, 16384]
    assert [sc.capacity(d) for d in (4, 16, 20, 128, 200, 256, 1504, 2048)] == [
        16, 16, 32, 128, 256, 256, 2048, 2048]
    # n <= 524,288: the lane groups the chunk pass holds, per capacity and generic
    assert [sc.chunk_groups(20000, c) for c in (16, 32, 64, 128, 256, 2048, None)] == [
        16384, 8192, 4096, 2048, 1024, 1024, 1024]
    # the combine pass: capped at 2,048 workgroups (4,096 generic) of 4 * GPW lane groups
    assert sc.combine_groups(2107400, 256) == 8192
    assert sc.combine_groups(16384 * 257, None) == 16384
    assert sc.combine_groups(1000, 256) == 4 * sc.cdiv(1000 // 256 + 2, 4)


# --- 1. every second-sweep shape crosses its threshold -------------------------------------------

def test_bag_ids_case_crosses():
    c = sc.bag_ids_case()
    assert sc.crosses_bag_ids(c["colptr"])
    assert c["B"] == sc.BAG_IDS_BAGS + 53 and set(np.unique(c["L"])) == {0, 1, 2}
    assert c["L"][0] == 0 and c["L"][-1] > 0 and len(c["values"]) == c["used"] + 7
    assert sc.multi_chunk_columns(c["values"], c["R"]) == c["R"]  # every column is multi-chunk
    assert not sc.crosses_bag_ids(c["colptr"][:sc.BAG_IDS_BAGS + 1])
    assert not sc.crosses_bag_ids(sc.small_ragged_case()["colptr"])


def test_apply_case_crosses():
    c = sc.apply_case()
    assert sc.crosses_apply(c["values"], c["R"])
    assert sc.distinct_columns(c["values"], c["R"]) == c["R"] == 70000
    assert c["B"] == 20000 and (c["L"] == 4).all()
    assert not sc.crosses_apply(c["values"][:sc.APPLY_COLUMNS], c["R"])


@pytest.mark.parametrize("name", sorted(sc.CHUNK_CASES))
def test_chunk_cases_cross(name):
    import test_gpu_adagrad as ta

    c = sc.chunk_case(name)
    cap = c["cap"]
    assert cap == (sc.capacity(c["D"]) if c["kind"] == "f32" and c["D"] % 4 == 0 else None)
    for values in (c["I"], c["values"]):  # the fixed-pool and the ragged form
        assert sc.crosses_chunks(values, c["R"], cap), name
        assert len(np.asarray(values).reshape(-1)) <= 524288  # the smallest grid
        cnt = sc.column_counts(values, c["R"])
        assert all(cnt[r] == n for r, n in ta.FORCED.items())
        touched = int((cnt > 0).sum()) - len(ta.FORCED)
        assert touched >= sc.CHUNK_CASES[name][2] and (cnt[1:] == 0).sum() >= 50
    assert same(c["values"][:c["n"]], c["I"].reshape(-1))
    assert int(c["colptr"][-1]) - 1 == c["n"] == len(c["values"]) - 7
    assert np.isnan(c["weights"][c["n"]:]).all() and not np.isnan(c["weights"][:c["n"]]).any()


@pytest.fixture(scope="module")
def combine():
    return sc.combine_case()


def test_combine_case_crosses(combine):
    c = combine
    assert sc.crosses_combine(c["values"], c["R"], sc.capacity(c["D"]))
    cnt = sc.column_counts(c["values"], c["R"])
    assert (cnt == 257).sum() == 8200 and (cnt[1:] == 0).sum() == 100
    assert len(c["values"]) == 2107400 and c["B"] == 4096 and c["L"].min() > 256
    # 8,192 multi-chunk columns fit one sweep: the predicate tells the two apart
    keep = np.isin(c["values"], np.unique(c["values"])[:8192])
    assert not sc.crosses_combine(c["values"][keep], c["R"], 256)


# --- 2. the sweeps reach everything they draw from -----------------------------------------------

def test_forward_sweep_coverage():
    cases = [sc.forward_case(s) for s in sc.FORWARD_SEEDS]
    assert len(cases) == 30
    seen = lambda key: {c[key] for c in cases}
    assert seen("family") == set(sc.FAMILIES)
    assert seen("B") == set(sc.FORWARD_B)
    assert seen("law") == set(sc.LAWS)
    assert seen("tail") == {0, 7} and seen("strided") == {False, True}
    assert seen("R") == set(sc.SWEEP_ROWS) and seen("D") == set(sc.SWEEP_DIMS)
    for family, kinds in sc.FORWARD_KINDS.items():
        mine = [c for c in cases if c["family"] == family]
        assert {c["kind"] for c in mine} == set(kinds), family
        assert {c["law"] for c in mine} == set(sc.LAWS), family
    floats = [c for c in cases if c["family"] in ("ragged", "wsum", "wmean")]
    assert {c["storage"] for c in floats} == set(sc.STORAGES)
    quants = [c for c in cases if c["family"] in ("int8", "int4")]
    assert {c["storage"] for c in quants} == {"fused_min", "fused_padded", "split_min",
                                              "split_padded"}
    assert {c["weight_grad"] for c in cases if c["family"] == "wsum"} == {False, True}
    assert any(c["B"] > sc.QUANT_REF_MAX_B for c in quants)
    for c in cases:
        assert c["used"] <= sc.MAX_ENTRIES and len(c["values"]) == c["used"] + c["tail"]
        assert c["values"].min(initial=1) >= 1 and c["values"].max(initial=1) <= c["R"]
        if c["family"] == "int4":
            assert c["D"] % 2 == 0
        if "rows" in c:
            assert c["rows"].shape == (c["R"], c["ld_bytes"]) and c["ld_bytes"] % 4 == 0
    assert any(c["law"] == "giant" and c["L"].max() == 3000 for c in cases)


def test_update_sweep_coverage():
    cases = [sc.update_case(s) for s in sc.UPDATE_SEEDS]
    assert len(cases) == 30
    seen = lambda key: {c[key] for c in cases}
    assert seen("opt") == set(sc.OPTIMISERS)
    assert seen("kind") == set(sc.UPDATE_KINDS)
    assert seen("storage") == set(sc.STORAGES)
    assert seen("B") == set(sc.UPDATE_B)
    assert seen("law") == set(sc.LAWS)
    assert seen("zipf") == {False, True} and seen("static") == {False, True}
    assert seen("R") == set(sc.SWEEP_ROWS) and seen("D") == set(sc.SWEEP_DIMS)
    ada = [c for c in cases if c["adagrad"]]
    assert len(ada) == 20 and 5 <= sum(c["fixed"] for c in ada) <= 9  # a third, about
    assert {c["fixed"] for c in ada if c["weighted"]} == {False, True}
    assert {c["fixed"] for c in ada if not c["weighted"]} == {False, True}
    for opt in sc.OPTIMISERS:
        assert len({c["kind"] for c in cases if c["opt"] == opt}) >= 3, opt
    for c in cases:
        assert c["used"] <= sc.MAX_ENTRIES and len(c["deltas"]) == (2 if c["adagrad"] else 1)
        assert not (c["fixed"] and not c["adagrad"])
        if c["fixed"]:
            assert (c["L"] == c["P"]).all() and c["tail"] == 0


def test_multi_sweep_coverage():
    cases = [sc.multi_case(s) for s in sc.MULTI_SEEDS]
    assert {c["kind"] for c in cases} == set(sc.UPDATE_KINDS)
    assert {c["k"] for c in cases} == set(sc.MULTI_PREPEND)
    assert {c["n"] for c in cases} >= {2, 5}
    assert {t["form"] for c in cases for t in c["tables"]} == set(sc.GRADIENTS)
    assert all(len({t["form"] for t in c["tables"]}) >= 2 for c in cases)
    for c in cases:
        assert c["delta"].shape == (c["B"], c["k"] + sum(t["D"] for t in c["tables"]))
        assert sum(t["used"] for t in c["tables"]) <= sc.MAX_ENTRIES


# --- 3. the vectorised equal-count AdaGrad reference is ref_step --------------------------------

@pytest.mark.parametrize("kname", ["f32", "bf16"])
@pytest.mark.parametrize("dim", [8, 7])
@pytest.mark.parametrize("count", [257, 513])
def test_equal_count_reference_is_ref_step(count, dim, kname):
    import test_gpu_adagrad as ta

    kind = ta.KINDS[kname]
    c = sc.combine_case(ncols=40, count=count, D=dim, R=60, B=37, kname=kname,
                        seed=[count, dim])
    assert (sc.column_counts(c["values"], 60) > 0).sum() == 40
    lists = ta.lists_ragged(c["values"], c["colptr"], nrows=60)
    cols, bagmat = sc.equal_count_lists(c["values"], c["colptr"], 60)
    assert sorted(lists) == cols.tolist()
    assert all(lists[col] == bagmat[i].tolist() for i, col in enumerate(cols))
    deltaC = kind.toC(c["delta"])
    g = sc.equal_count_g(deltaC, bagmat)
    for i, col in enumerate(cols):
        assert same(g[i], ta.ref_g(deltaC, lists[col])), col
    t1, s1 = c["table"].copy(), c["state"].copy()
    t2, s2 = c["table"].copy(), c["state"].copy()
    ta.ref_step(kind, t1, s1, c["delta"], lists)
    sc.equal_count_step(kind, t2, s2, c["delta"], c["values"], c["colptr"])
    assert same(t1, t2) and same(s1, s2)
    assert not same(t1, c["table"]) and not same(s1, c["state"])
    untouched = np.setdiff1d(np.arange(60), cols)
    assert len(untouched) == 20 and same(t2[untouched], c["table"][untouched])


def test_equal_count_reference_with_uncovered_entries():
    """Entries no bag covers keep their list position and add nothing: the same values under
    a colptr that starts 30 entries in and ends 45 entries early."""
    import test_gpu_adagrad as ta

    kind = ta.KINDS["f32"]
    c = sc.combine_case(ncols=40, count=257, D=8, R=60, B=37, seed=5)
    colptr = c["colptr"].copy()
    colptr[1:] = np.clip(colptr[1:], 31, len(c["values"]) - 44)
    colptr[0] = 31
    lists = ta.lists_ragged(c["values"], colptr, nrows=60)
    assert sum(b == 0 for bags in lists.values() for b in bags) == 75
    t1, s1 = c["table"].copy(), c["state"].copy()
    t2, s2 = c["table"].copy(), c["state"].copy()
    ta.ref_step(kind, t1, s1, c["delta"], lists)
    sc.equal_count_step(kind, t2, s2, c["delta"], c["values"], colptr)
    assert same(t1, t2) and same(s1, s2)
