"""The chain plans of the DEFAULT (exact) sparse SGD on long runs and on both sides of every
threshold between its three planners (embeddingtables.jl_amd/csrc/et_update.hip).

A column of more than ET_SGD_CHUNK occurrences is summed as a serial chain, planned by
  * the early chains (EC: `ec_table`, tables of at most 128 rows, pool <= 255, batch <= 2^20),
  * the early hot columns (EH: `eh_table`, at most 16 candidates per larger table, picked by
    `k_eh_pick` from a sample of the first 1,024 bags), or
  * the regular plan (`k_chain_tile_count` / `k_chain_tcount` / `k_chain_choose` /
    `k_chain_emit`: tiles of 4,096 occurrences staged in LDS with a halo of 64; a run of r
    occurrences of one column in one bag is credited to the tile where it starts and followed
    into global memory past the halo, `run_length`).
Part A puts long runs at chosen places of the regular plan's tiles, in every element type, on
paged and column-pointer tables, behind odd occurrence offsets and through the two-phase
update.  Part B runs one draw on both sides of each early-path threshold; "twice" cases also
repeat bit for bit, since their candidate choice depends on atomic arrival order and the sum
must not.  Part C does the same for the split mode's hot pass (`hot_shape`).

The reference is the C oracle (oracle.sgd / oracle.sgd_multi: the reference's serial sum from
+0 in occurrence order, then fma(-eta, acc, w), src/sparseupdate.jl:110-127).  Every column of
every table is compared byte for byte.  tests/test_sgd_threshold_cases_host.py proves on the
host that each case has the shape named here."""
import numpy as np
import pytest
import torch

import embtab as et
import sgd_threshold_cases as tc
from embtab import _lib
from embtab.tables import Static, fused_update_path
from test_gpu_paged_chains import ColumnPointerTable
from test_gpu_update import _dev_typed, _fp64_update_and_scale, _host_bits, _typed

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ETA = 0.1

# et_update.hip, mirrored here and in tests/sgd_threshold_cases.py
CHUNK = _lib.ET_SGD_CHUNK    # include/embtab.h; kExactChunk: a longer column is a chain
CHAIN_TILE = 4096            # :1192 kChainTile
CHAIN_HALO = 64              # :1201 kChainHalo
EC_MAX_ROWS = 128            # :1636 kEcMaxRows
EC_MAX_POOL = 255            # :1638 kEcMaxPool
EC_MAX_BATCH = 1 << 20       # :1639 kEcMaxBatch
EH_SAMPLE_BAGS = 1024        # :1651 kEhSampleBags
EH_MIN_OCC = 32768           # :1652 kEhMinOcc (the test is hc * batch >= min_occ * nb, :1727)
EH_K = 16                    # :1285 kEhK
EH_QUALIFY = 512             # :1687 qk / qc, filled at :1729
EH_HASH, EH_PROBES = 4096, 16  # :1653 kEhHash, :1654 kEhProbes
HOT_MAX_POOL = 32            # :869 kHotMaxPool (hot_shape, :2437)


def test_constants_are_the_case_builders():
    assert CHUNK == tc.CHUNK == 256
    assert (CHAIN_TILE, CHAIN_HALO) == (tc.TILE, tc.HALO)
    assert (EC_MAX_ROWS, EC_MAX_POOL, EC_MAX_BATCH) == (tc.EC_MAX_ROWS, tc.EC_MAX_POOL,
                                                        tc.EC_MAX_BATCH)
    assert (EH_SAMPLE_BAGS, EH_MIN_OCC, EH_K, EH_QUALIFY, EH_HASH, EH_PROBES) == (
        tc.EH_SAMPLE_BAGS, tc.EH_MIN_OCC, tc.EH_K, tc.EH_QUALIFY, tc.EH_HASH, tc.EH_PROBES)
    assert HOT_MAX_POOL == tc.HOT_MAX_POOL


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def simple(x):
    return et.SimpleEmbedding(dev(x), Static(x.shape[1]))


def dense(A):
    if isinstance(A, et.SimpleEmbedding):
        return A.data
    return A.to_dense() if isinstance(A, et.SplitEmbedding) else A.dense()


def oracle_sgd(oracle, table, delta, I):
    """The oracle's update of a copy of `table` (Float32, the fused path of a Static(16))."""
    ref = table.copy()
    oracle.sgd(ref, np.ascontiguousarray(delta), I, ETA, fused=True)
    return ref


def update_one(table, delta, I, make=simple):
    """et.update_ in the default mode on a fresh table; the whole table as numpy."""
    A = make(table)
    assert fused_update_path(A)
    et.update_(et.Descent(ETA), A, et.SparseEmbeddingUpdate(A.lookup_type, dev(delta), dev(I)))
    torch.cuda.synchronize()
    return dense(A).cpu().numpy()


def update_many(tables, delta, offs, idx, batches=None):
    """One multi-table et.update_ (default mode) whose gradients are column blocks of one
    gradient; table t reads its first batches[t] rows.  The whole tables as numpy."""
    tabs = [simple(x) for x in tables]
    dd = delta if isinstance(delta, torch.Tensor) else dev(delta)
    grads = []
    for t, (A, o, I) in enumerate(zip(tabs, offs, idx)):
        B = len(I) if batches is None else batches[t]
        grads.append(et.SparseEmbeddingUpdate(A.lookup_type, dd[:B, o:o + A.data.shape[1]],
                                              dev(I)))
    et.update_(et.Descent(ETA), tabs, grads)
    torch.cuda.synchronize()
    return [A.data.cpu().numpy() for A in tabs]


def check_pair(oracle, tables, delta, idx, twice=False):
    """The tables of one call, each a DIM-wide block of `delta`, against the oracle; `twice`:
    a second call on fresh tables gives the same bytes."""
    offs = [tc.DIM * t for t in range(len(tables))]
    got = update_many(tables, delta, offs, idx)
    host = delta.cpu().numpy() if isinstance(delta, torch.Tensor) else delta
    for t, (x, I) in enumerate(zip(tables, idx)):
        ref = oracle_sgd(oracle, x, host[:len(I), offs[t]:offs[t] + tc.DIM], I)
        assert same(got[t], ref), f"table {t}"
        assert not same(got[t], x)
    if twice:
        again = update_many(tables, delta, offs, idx)
        assert all(same(a, b) for a, b in zip(got, again))
    assert et.check_errors() == 0


# --- A. long runs in the regular plan ------------------------------------------------------------

@pytest.fixture(scope="module")
def halo_ref(oracle):
    """The oracle's Float32 update of halo_case, shared by the tests that run that case."""
    c = tc.halo_case()
    ref = oracle_sgd(oracle, c["table"], c["delta"], c["I"])
    ref.setflags(write=False)
    return ref


def test_halo_and_tile_alignment(halo_ref):
    """A1.  200 rows, 300 bags of 100 (no EC: 200 rows; no EH candidate: every column below
    32,768).  Column H's runs: lengths 1, 15, 16, 17, 63, 64, 65, 66 and 100; a head on a
    tile's first slot and a run ending on a tile's last; heads on the last slots of three
    tiles with 64 (ends with the halo), 65 (the last staged slot) and 66 occurrences (one in
    global memory); a run of 100 with 6 occurrences before a tile boundary and 94 after.
    Column G: runs of 17..40, all inside the halo."""
    et.check_errors()
    c = tc.halo_case()
    got = update_one(c["table"], c["delta"], c["I"])
    assert same(got, halo_ref)
    assert not same(got[c["H"] - 1], c["table"][c["H"] - 1])
    assert et.check_errors() == 0


@pytest.mark.parametrize("P", [256, 300])
def test_pool_above_255_on_a_tiny_table(oracle, P):
    """A2.  3 rows, 64 bags of 256 / 300: the early chains refuse the pool (one byte per
    per-bag count), so a 3-row table's runs of ~140 and one of 256 / 300 go through the
    regular plan, each outlasting the halo."""
    et.check_errors()
    c = tc.tiny_pool_case(P)
    got = update_one(c["table"], c["delta"], c["I"])
    assert same(got, oracle_sgd(oracle, c["table"], c["delta"], c["I"]))
    assert et.check_errors() == 0


def test_run_longer_than_a_tile(oracle):
    """A3.  3 rows, 12 bags of 5,000: a bag that is one column throughout (a run of 5,000:
    one tile of the column holds no head), 4,000 of the same column in the bags around it,
    and the last column's last run (4,500) ending with the sorted occurrences."""
    et.check_errors()
    c = tc.long_run_case()
    got = update_one(c["table"], c["delta"], c["I"])
    assert same(got, oracle_sgd(oracle, c["table"], c["delta"], c["I"]))
    assert et.check_errors() == 0


@pytest.mark.parametrize("kind", ["f64", "f16", "f16acc", "bf16"])
def test_halo_case_other_element_types(oracle, kind):
    """A4.  halo_case's indices on Float64 / Float16 (with and without Float32 sums) /
    BFloat16 tables: chain_walk_wide, which reads an entry's r and bag through chain_shift.
    Bit-identical to the oracle's typed model of the reference's update."""
    et.check_errors()
    c = tc.halo_case()
    rng = np.random.default_rng(0xA4)
    base = _typed(rng, (c["R"], tc.DIM), kind)
    delta = _typed(rng, (c["B"], tc.DIM), kind)
    A = et.SimpleEmbedding(_dev_typed(base, kind), Static(tc.DIM))
    g = et.SparseEmbeddingUpdate(A.lookup_type, _dev_typed(delta, kind), dev(c["I"]))
    et.update_(et.Descent(ETA), A, g, f16_fp32_acc=kind == "f16acc")
    torch.cuda.synchronize()
    ref = base.copy()
    oracle.sgd(ref, delta, c["I"], ETA, fused=fused_update_path(A), bf16=kind == "bf16",
               f16_fp32_acc=kind == "f16acc")
    got = _host_bits(A.data)
    assert same(got, ref.view(got.dtype))
    assert not same(got[c["H"] - 1], base.view(got.dtype)[c["H"] - 1])
    assert et.check_errors() == 0


@pytest.mark.parametrize("storage", ["paged", "colptr"])
def test_halo_case_other_storage(halo_ref, storage):
    """A5.  halo_case on a paged table (7 columns per page) and through a device
    column-pointer array."""
    et.check_errors()
    c = tc.halo_case()
    gen = torch.Generator(device=DEV)
    gen.manual_seed(0xA5)

    def make(x):
        t = dev(x)
        A = et.SplitEmbedding(t, 7) if storage == "paged" else ColumnPointerTable(
            t, tc.DIM + 4, gen)
        assert A.device_table()[1] == (7 if storage == "paged" else 1)
        return A

    assert same(update_one(c["table"], c["delta"], c["I"], make), halo_ref)
    assert et.check_errors() == 0


def test_long_runs_behind_odd_occurrence_offsets(oracle):
    """A6.  A 5-row, pool-7 table of 129 bags, then the tables of A1, A2 (pool 300) and A3 in
    one call: their occurrence offsets 903, 30,903 and 50,103 are odd and no multiple of a
    pool (bag = (position - occ_off) / pool); the gradients are blocks of one gradient with 3
    prepended columns.  Against oracle.sgd_multi."""
    et.check_errors()
    c = tc.offsets_case()
    tabs = c["tables"]
    got = update_many([t["table"] for t in tabs], c["delta"], c["offs"],
                      [t["I"] for t in tabs], [t["B"] for t in tabs])
    refs = [t["table"].copy() for t in tabs]
    oracle.sgd_multi(refs, c["delta"], [t["I"] for t in tabs], ETA, [True] * len(tabs),
                     num_splits=4, nthreads=4, delta_offsets=c["offs"])
    for t in range(len(tabs)):
        assert same(got[t], refs[t]), f"table {t}"
        assert not same(got[t], tabs[t]["table"])
    assert et.check_errors() == 0


def test_halo_case_two_phase_update(halo_ref):
    """A7.  halo_case through PhasedUpdate: the index phase on a side stream, then the
    update phase; the index array may be overwritten in between."""
    et.check_errors()
    c = tc.halo_case()
    A = simple(c["table"])
    I = dev(c["I"])
    pu = et.PhasedUpdate([A], [et.SparseEmbeddingUpdate(A.lookup_type, dev(c["delta"]), I)])
    main, side = torch.cuda.current_stream(), torch.cuda.Stream()
    side.wait_stream(main)
    pu.index_(side)
    main.wait_stream(side)
    I.fill_(1)  # the update phase never reads the indices again
    pu.update_(et.Descent(ETA))
    torch.cuda.synchronize()
    assert same(A.data.cpu().numpy(), halo_ref)
    assert et.check_errors() == 0


# --- B. both sides of every early-path threshold -------------------------------------------------

@pytest.mark.parametrize("P", [255, 256])
def test_pool_255_and_256(oracle, P):
    """B1.  A 3-row and a 1,000-row table, 300 bags: at pool 255 the small table's chains are
    early chains (one bag is a single column: a byte counter of 255) and the large table's
    45 % column (at least 32,768 occurrences) an early hot column; at pool 256, the same draw
    with one more index per bag, both tables go through the regular plan."""
    et.check_errors()
    c = tc.pool_pair_case()
    check_pair(oracle, c["tables"], c["delta"], [I[:, :P] for I in c["I"]])


@pytest.fixture(scope="module")
def batch_pair():
    c = tc.batch_pair_case()
    yield c
    c.clear()


@pytest.mark.parametrize("B", [1 << 20, (1 << 20) + 1])
def test_batch_2_pow_20_and_one_more(oracle, batch_pair, B):
    """B2.  Pool 1, a 3-row and a 1,000-row table.  In every 1,024 bags of the large table
    column X occurs 32 times (32 * 2^20 = 32,768 * 1,024: a candidate, the test is >=), Y 31
    times (no candidate: a regular chain of 31,744) and W 60 times.  At 2^20 + 1 bags neither
    table is early."""
    et.check_errors()
    c = batch_pair
    check_pair(oracle, c["tables"], c["delta"][:B], [I[:B] for I in c["I"]])
    torch.cuda.empty_cache()


@pytest.mark.parametrize("B", [1023, 1024, 1025])
def test_sample_is_the_whole_batch(oracle, B):
    """B3.  Pool 40, two 1,000-row tables (an 85 % and a 70 % column cannot share a table):
    one column at 85 % (at least 32,768 occurrences at all three sizes: an early hot column)
    and one at 70 % (below 32,768: a regular chain).  Up to 1,024 bags the sample is the
    whole batch; at 1,025 it is a part, scaled by batch / 1,024."""
    et.check_errors()
    c = tc.sample_case()
    check_pair(oracle, c["tables"], c["delta"][:B], [I[:B] for I in c["I"]])


def test_candidate_that_is_not_a_chain(oracle):
    """B4.  131,072 bags, pool 1.  X: 256 occurrences, all sampled: a candidate
    (256 * 131,072 = 32,768 * 1,024) but no chain, the chunk pass takes it.  Y: 257, likewise:
    an early hot chain of 257.  Z: 40,000, none sampled: a regular chain."""
    et.check_errors()
    c = tc.not_a_chain_case()
    check_pair(oracle, [c["table"]], c["delta"], [c["I"]])


def test_more_candidates_than_slots_with_ties(oracle):
    """B5.  131,072 bags, 1,000 rows: 20 columns with the same sample count above the
    candidate threshold; 16 become early hot chains (ties to the smaller column), 4 regular
    chains.  The pool is 8: at this batch the threshold is 256 sampled occurrences, and 20
    columns of 256 do not fit the 4,096 sampled slots of a pool of 4.  Twice."""
    et.check_errors()
    c = tc.tie_case()
    check_pair(oracle, [c["table"]], c["delta"], [c["I"]], twice=True)


def test_more_than_512_qualifying_columns(oracle):
    """B6.  2^20 bags of 20, 700 rows: 600 columns occur 33 times each in every 1,024 bags
    (threshold 32), more than k_eh_pick's buffer of 512 qualifying columns, so which 512 are
    ranked depends on arrival order; whichever 16 become early hot chains, the other
    multi-chunk columns are regular chains.  21 M occurrences; the gradient is filled on the
    device.  Twice."""
    et.check_errors()
    c = tc.qualify_case()
    delta = torch.empty((c["B"], tc.DIM), dtype=torch.float32, device=DEV)
    _lib.check(_lib.load().et_fill_uniform(_lib.ET_F32, delta.data_ptr(), delta.numel(), 0xB6, 0,
                                           -1.0, 1.0, _lib.stream_handle()))
    check_pair(oracle, [c["table"]], delta, [c["I"]], twice=True)
    del delta
    torch.cuda.empty_cache()


def test_crowded_sample_hash(oracle):
    """B7.  100,000 rows, 4,096 bags of 20, uniform but for one column with a 45 % share: the
    sample holds over 8,192 distinct columns for 4,096 hash slots, so occurrences are dropped
    after 16 probes and what is counted depends on arrival order.  Twice."""
    et.check_errors()
    c = tc.crowded_case()
    check_pair(oracle, [c["table"]], c["delta"], [c["I"]], twice=True)


# --- C. split-mode hot pass, pool 32 | 33 --------------------------------------------------------

def _split_update(table, delta, I, hot_pass):
    A = simple(table)
    g = et.SparseEmbeddingUpdate(A.lookup_type, dev(delta), dev(I))
    et.update_(et.Descent(ETA), A, g, exact=False, hot_pass=hot_pass)
    torch.cuda.synchronize()
    return A.data.cpu().numpy()


@pytest.mark.parametrize("P,D", [(32, 128), (33, 128), (32, 124)])
def test_hot_pass_pool_32_and_33(oracle, P, D):
    """C.  dim 128, 1,500 bags, 300 rows, the split mode (exact=False: the exact mode has no
    hot pass) with hot_pass=True.  hot_shape holds at pool 32 and not at pool 33 or dim 124.
    Columns of at most 256 occurrences are bit-identical to the oracle, longer ones within
    1e-6 of the summation scale, and the result repeats.  Where the table is not hot-shaped
    the flag changes nothing, bit for bit; where it is, the multi-chunk columns are summed in
    another order than the plain split mode's (1,024-bag windows, not 256-occurrence chunks),
    which shows in their bits."""
    et.check_errors()
    c = tc.hot_pass_case()
    table = np.ascontiguousarray(c["table"][:, :D])
    delta = np.ascontiguousarray(c["delta"][:, :D])
    I = np.ascontiguousarray(c["I"][:, :P])
    got = _split_update(table, delta, I, True)
    assert same(got, _split_update(table, delta, I, True))
    ref = table.copy()
    oracle.sgd(ref, delta, I, ETA, fused=True)
    short = tc.column_counts(I, c["R"])[1:] <= CHUNK
    assert short.any() and not short.all()
    assert same(got[short], ref[short])
    exact_upd, scale = _fp64_update_and_scale(table, delta, I, ETA)
    assert np.all(np.abs(got.astype(np.float64) - exact_upd) <= 1e-6 * scale)
    plain = _split_update(table, delta, I, False)
    assert same(got, plain) == (not (D == 128 and P <= HOT_MAX_POOL))
    assert et.check_errors() == 0
