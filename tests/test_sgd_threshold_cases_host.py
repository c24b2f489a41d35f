"""The parts of tests/test_gpu_sgd_thresholds.py that need no GPU: every case of
tests/sgd_threshold_cases.py is shown to have the shape it claims (run heads and lengths against
the regular plan's tiles and halo, sample counts against k_eh_pick's candidate test, its
qualifying buffer and its hash), and et_sgd_workspace_size — pure host code that sizes the
early-chain, hot-column and hot-pass buffers whatever the flags — is shown to step exactly at
the thresholds the cases assume: pool 255 | 256, batch 2^20 | 2^20 + 1, 128 | 129 rows and
(dim 128) pool 32 | 33."""
import ctypes

import numpy as np
import pytest

import sgd_threshold_cases as tc

T, HALO, CHUNK = tc.TILE, tc.HALO, tc.CHUNK


def test_chunk_constant_is_the_library_header():
    from embtab import _lib

    assert tc.CHUNK == _lib.ET_SGD_CHUNK == 256


def no_eh_candidate(I, R):
    I = tc.as_matrix(I)
    assert len(I) <= tc.EH_SAMPLE_BAGS  # the sample is the whole batch
    return tc.column_counts(I, R)[1:].max() < tc.EH_MIN_OCC and len(tc.eh_qualifying(I, R)) == 0


# --- A. long runs in the regular plan ------------------------------------------------------------

def test_halo_case_shapes():
    c = tc.halo_case()
    I, R, B, P = c["I"], c["R"], c["B"], c["P"]
    assert (R, B, P) == (200, 300, 100) and I.shape == (B, P)
    assert I.min() >= 1 and I.max() <= R
    assert not tc.ec_table(R, P, B) and tc.eh_table(R, P, B)
    assert no_eh_candidate(I, R)  # so H and G are chains of the regular plan
    heads, r = tc.runs_of(I, c["H"])
    total = int(r.sum())
    assert CHUNK < total < tc.EH_MIN_OCC and total > 5 * T
    assert r.tolist() == tc.halo_h_runs()
    assert {1, 15, 16, 17, 63, 64, 65, 66, 100} <= set(r.tolist())
    ends = heads + r  # one past a run's last occurrence
    first = np.flatnonzero((heads % T == 0) & (heads > 0))
    assert len(first) and r[first[0]] == 100            # a head on a tile's first slot
    assert ((ends % T == 0) & (ends < total)).any()     # a run ending on a tile's last slot
    last_slot = {int(h) // T: int(n) for h, n in zip(heads, r) if h % T == T - 1}
    assert last_slot == {1: 64, 2: 65, 3: 66}           # heads on three tiles' last slots
    # 64: slots 4096..4159 of stage_bags, the whole halo; 65: the last staged slot as well;
    # 66: one occurrence beyond LDS (run_length's global-memory branch)
    six = np.flatnonzero((r == 100) & (heads % T == T - 6))
    assert len(six) == 1 and heads[six[0]] // T == 4    # 6 before the boundary, 94 after
    assert (r[(heads % T) + r > T + HALO] > HALO).any()
    # the runs are scattered in their bags, not sorted
    rows = I[(I == c["H"]).sum(1) > 1]
    assert any((np.diff(np.flatnonzero(row == c["H"])) > 1).any() for row in rows)
    assert not any((np.diff(row) >= 0).all() for row in I if (row != row[0]).any())
    # G: a chain whose runs all end inside the halo
    _, g = tc.runs_of(I, c["G"])
    assert g.sum() > CHUNK and g.min() == 17 and g.max() == 40 and set(g.tolist()) == set(
        range(17, 41))
    # S = 16 is the plan's choice for H (entries x cost), so runs above 16 leave remainders
    cost = {1: 9, 2: 17, 4: 21, 8: 22, 16: 38}  # chain_entry_cost2
    E = {S: int(np.ceil(r / S).sum()) for S in cost}
    assert min(cost, key=lambda S: (E[S] * cost[S], S)) == 16 and (r[r > 16] % 16 != 0).any()


@pytest.mark.parametrize("P", [256, 300])
def test_tiny_pool_case_shapes(P):
    c = tc.tiny_pool_case(P)
    I = c["I"]
    assert (c["R"], c["B"]) == (3, 64) and I.shape == (64, P) and P > tc.EC_MAX_POOL
    assert not tc.ec_table(3, P, 64) and not tc.eh_table(3, P, 64)
    assert tc.ec_table(3, tc.EC_MAX_POOL, 64)
    assert (I[c["full_bag"]] == c["full_col"]).all()
    cnt = tc.column_counts(I, 3)[1:]
    assert (cnt > CHUNK).all()  # three chains
    _, r = tc.runs_of(I, c["full_col"])
    assert r.max() == P and (r > HALO).sum() == 64  # every run leaves the staged bags


def test_long_run_case_shapes():
    c = tc.long_run_case()
    I, B, P = c["I"], c["B"], c["P"]
    assert (c["R"], B, P) == (3, 12, 5000) and not tc.ec_table(3, P, B)
    heads, r = tc.runs_of(I, 1)
    assert r[:3].tolist() == [4000, 5000, 4000] and heads[:3].tolist() == [0, 4000, 9000]
    assert (I[1] == 1).all()
    assert 1 in tc.tiles_without_head(heads, int(r.sum()))  # tile 1: no run starts in it
    # column 3 is the last key, so its list ends where the sorted occurrences end (n)
    n = B * P
    cnt = tc.column_counts(I, 3)
    assert cnt[1:].sum() == n and cnt[3] > 0
    h3, r3 = tc.runs_of(I, 3)
    assert (I[B - 1] == 3).sum() == r3[-1] == 4500 and h3[-1] + r3[-1] == cnt[3]
    assert r3[-1] > T + HALO


def test_offsets_case_shapes():
    c = tc.offsets_case()
    tabs = c["tables"]
    assert [(t["R"], t["P"]) for t in tabs] == [(5, 7), (200, 100), (3, 300), (3, 5000)]
    assert c["occ_off"] == [0, 903, 30903, 50103]
    for off in c["occ_off"][1:]:
        # bag = (position - occ_off) / pool: odd, and no multiple of a pool it is divided by
        assert off % 2 == 1 and all(off % u["P"] for u in tabs[1:])
    assert tc.ec_table(5, 7, 129)
    assert c["delta"].shape == (300, 3 + 4 * tc.DIM) and c["offs"] == [3, 19, 35, 51]
    assert all(t["B"] <= 300 for t in tabs)


# --- B. both sides of every early-path threshold -------------------------------------------------

def test_pool_pair_case_shapes():
    c = tc.pool_pair_case()
    B = c["B"]
    for P, early in ((255, True), (256, False)):
        small, large = (I[:, :P] for I in c["I"])
        assert tc.ec_table(3, P, B) == early and tc.eh_table(1000, P, B) == early
        assert (small[41] == 3).all()  # r = pool: 255 is a byte's largest value
        cnt = tc.column_counts(large, 1000)
        assert cnt[c["hot"]] >= tc.EH_MIN_OCC
        assert tc.eh_qualifying(large, 1000).tolist() == [c["hot"]]
        assert CHUNK < cnt[77] < tc.EH_MIN_OCC  # a regular chain on both sides
        assert (tc.column_counts(small, 3)[1:] > CHUNK).all()


def test_batch_pair_case_shapes():
    c = tc.batch_pair_case()
    assert c["B"] == tc.EC_MAX_BATCH + 1
    large = c["I"][1]
    for B, early in ((tc.EC_MAX_BATCH, True), (tc.EC_MAX_BATCH + 1, False)):
        assert tc.ec_table(3, 1, B) == early and tc.eh_table(1000, 1, B) == early
    B = tc.EC_MAX_BATCH
    s = tc.sample_counts(large[:B], 1000)
    assert (s[tc.BATCH_X], s[tc.BATCH_Y], s[tc.BATCH_W]) == (32, 31, 60)
    assert 32 * B == tc.EH_MIN_OCC * 1024  # the test is >=: X is a candidate, Y is not
    assert tc.eh_qualifying(large[:B], 1000).tolist() == sorted([tc.BATCH_X, tc.BATCH_W])
    per_block = large[:B].reshape(-1, 1024)
    for col, n in ((tc.BATCH_X, 32), (tc.BATCH_Y, 31), (tc.BATCH_W, 60)):
        assert ((per_block == col).sum(1) == n).all()  # the same rate through the batch
    cnt = tc.column_counts(large[:B], 1000)
    assert cnt[tc.BATCH_Y] == 31 * 1024 > CHUNK  # Y: a regular chain
    assert (tc.column_counts(c["I"][0], 3)[1:] > CHUNK).all()
    assert tc.hash_longest_cluster(large[:B], 1000) <= tc.EH_PROBES


def test_sample_case_shapes():
    c = tc.sample_case()
    for B in (1023, 1024, 1025):
        assert tc.eh_table(1000, 40, B)
        (a, ca), (b, cb) = ((I[:B], col) for I, col in zip(c["I"], c["hot"]))
        assert tc.column_counts(a, 1000)[ca] >= tc.EH_MIN_OCC
        assert CHUNK < tc.column_counts(b, 1000)[cb] < tc.EH_MIN_OCC
        assert tc.eh_qualifying(a, 1000).tolist() == [ca]
        assert tc.eh_qualifying(b, 1000).tolist() == []
    assert min(1025, tc.EH_SAMPLE_BAGS) == 1024  # only the largest side samples a part


def test_not_a_chain_case_shapes():
    c = tc.not_a_chain_case()
    I, B = c["I"], c["B"]
    assert B == 131072 and I.shape == (B,)
    cnt, s = tc.column_counts(I, 1000), tc.sample_counts(I, 1000)
    assert (cnt[tc.NAC_X], cnt[tc.NAC_Y], cnt[tc.NAC_Z]) == (256, 257, 40000)
    assert (s[tc.NAC_X], s[tc.NAC_Y], s[tc.NAC_Z]) == (256, 257, 0)
    assert 256 * B == tc.EH_MIN_OCC * 1024
    assert tc.eh_pick(I, 1000).tolist() == [tc.NAC_X, tc.NAC_Y]
    assert cnt[tc.NAC_X] == CHUNK and cnt[tc.NAC_Y] == CHUNK + 1  # chunk pass | EH chain
    assert tc.hash_longest_cluster(I, 1000) <= tc.EH_PROBES


def test_tie_case_shapes():
    c = tc.tie_case()
    I, B = c["I"], c["B"]
    assert I.shape == (131072, tc.TIE_POOL)
    # 20 columns at the candidate threshold of 256 need 20 * 256 = 5,120 sampled slots: a
    # pool of 4 (4,096 slots) cannot hold them, hence the pool of 8
    assert tc.eh_qualifies(256, B) and not tc.eh_qualifies(255, B)
    assert 20 * 256 > 1024 * 4 and 20 * tc.TIE_COUNT <= 1024 * tc.TIE_POOL
    s = tc.sample_counts(I, 1000)
    assert all(s[col] == tc.TIE_COUNT for col in tc.TIE_COLS)
    q = tc.eh_qualifying(I, 1000)
    assert q.tolist() == list(tc.TIE_COLS) and len(q) == 20 > tc.EH_K
    assert tc.hash_longest_cluster(I, 1000) <= tc.EH_PROBES  # the counts are exact
    assert tc.eh_pick(I, 1000).tolist() == list(tc.TIE_COLS[:tc.EH_K])  # ties: smaller column
    cnt = tc.column_counts(I, 1000)
    assert all(cnt[col] == tc.TIE_COUNT * 128 > tc.EH_MIN_OCC for col in tc.TIE_COLS)


def test_qualify_case_shapes():
    c = tc.qualify_case()
    I, B = c["I"], c["B"]
    assert I.shape == (1 << 20, 20) and c["R"] == 700 and tc.eh_table(700, 20, B)
    s = tc.sample_counts(I, 700)
    assert (s[1:tc.QUALIFY_COLS + 1] == 33).all() and 33 * 600 == 19800
    assert tc.eh_qualifies(33, B) and not tc.eh_qualifies(31, B)
    assert tc.hash_longest_cluster(I, 700) <= tc.EH_PROBES
    assert len(tc.eh_qualifying(I, 700)) >= tc.QUALIFY_COLS > tc.EH_QUALIFY
    cnt = tc.column_counts(I, 700)
    assert (cnt[1:tc.QUALIFY_COLS + 1] == 33 * 1024).all()  # the same rate through the batch


def test_crowded_case_shapes():
    c = tc.crowded_case()
    I, R = c["I"], c["R"]
    assert I.shape == (4096, 20) and R == 100000 and tc.eh_table(R, 20, 4096)
    s = tc.sample_counts(I, R)
    assert (s > 0).sum() > 2 * tc.EH_HASH  # far more sampled columns than hash slots
    assert tc.hash_longest_cluster(I, R) == tc.EH_HASH
    cnt = tc.column_counts(I, R)
    assert cnt[c["hot"]] >= tc.EH_MIN_OCC and tc.eh_qualifies(s[c["hot"]], 4096)
    assert np.sort(cnt)[-2] < CHUNK  # every other column goes through the chunk pass


def test_hot_pass_case_shapes():
    c = tc.hot_pass_case()
    assert (c["B"], c["R"], c["P"], c["D"]) == (1500, 300, 33, 128)
    for P in (32, 33):
        cnt = tc.column_counts(c["I"][:, :P], 300)[1:]
        assert (cnt > CHUNK).sum() >= 3 and ((cnt > 0) & (cnt <= CHUNK)).sum() >= 100
        assert (cnt > CHUNK).sum() <= 120  # kHotSlots: every multi-chunk column goes hot


# --- the library's own thresholds, from et_sgd_workspace_size ------------------------------------

def workspace_size(nrows, dim, pool, batch):
    from embtab import _lib

    P = 1 << 20  # a 16-byte aligned stand-in for device memory: the size call reads no memory
    d = (_lib.UpdateDesc * 1)(_lib.UpdateDesc(P, dim, nrows, dim, pool, 2 * P, dim, 3 * P, pool,
                                              batch, 0))
    nb = ctypes.c_int64(0)
    assert _lib.load().et_sgd_workspace_size(ctypes.addressof(d), 1, ctypes.byref(nb)) == 0
    return nb.value


THRESHOLDS = {
    # name: (the last value on the near side, size as a function of the varied quantity)
    "pool 255|256, 3 rows": (255, lambda p: workspace_size(3, 16, p, 300)),
    "pool 255|256, 1000 rows": (255, lambda p: workspace_size(1000, 16, p, 300)),
    "batch 2^20|2^20+1, 3 rows": (1 << 20, lambda b: workspace_size(3, 16, 1, b)),
    "batch 2^20|2^20+1, 1000 rows": (1 << 20, lambda b: workspace_size(1000, 16, 1, b)),
    "rows 128|129": (128, lambda r: workspace_size(r, 16, 20, 4096)),
    "dim 128, pool 32|33": (32, lambda p: workspace_size(300, 128, p, 1500)),
}


@pytest.mark.parametrize("name", sorted(THRESHOLDS))
def test_workspace_size_steps_at_the_threshold(name):
    """size(x + 1) - size(x) for the three units before and after the threshold: the six
    ordinary steps agree within the layout's 256-byte rounding of each buffer, the step
    across the threshold (buffers appear or vanish) is far outside their range."""
    at, size = THRESHOLDS[name]
    sizes = [size(x) for x in range(at - 3, at + 5)]
    steps = np.diff(sizes)
    across, ordinary = int(steps[3]), np.delete(steps, 3)
    spread = int(ordinary.max() - ordinary.min())
    assert spread <= 64 * 256, (name, steps)  # fewer than 64 buffers, each rounded to 256
    gap = min(abs(across - int(o)) for o in ordinary)
    assert gap > 4 * (spread + 256), (name, steps)


def test_workspace_size_without_a_threshold_has_no_step():
    """The control: the same probe finds nothing at pool 250|251 or at dim 124, pool 32|33."""
    for at, size in ((250, lambda p: workspace_size(3, 16, p, 300)),
                     (32, lambda p: workspace_size(300, 124, p, 1500))):
        steps = np.diff([size(x) for x in range(at - 3, at + 5)])
        assert steps.max() - steps.min() <= 64 * 256, steps
