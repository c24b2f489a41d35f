"""The split sparse SGD over ragged and weighted gradients on the GPU (et_ragged_sgd_split
through ``et.update_(Descent, ..., split=True)``), bit for bit against the numpy restatement of
the contract in tests/ragged_split_ref.py (``tobytes()`` equality throughout, no tolerance).

Inputs (``ragged_split_ref.split_case``): tables of 1,000 rows, 300 bags of mixed lengths with
empty ones, a hot row of 3,000 covered entries in ten bags (12 chunks with the three uncovered
entries in front of ``colptr[0]`` that name it too), rows of exactly 255, 256, 257, 512 and 513
entries, and a capacity tail of valid indices.  tests/test_ragged_split_host.py shows in numpy
that on these inputs the chunked sum differs from the serial one in the hot column and nowhere
among the columns of at most ET_SGD_CHUNK entries."""
import ctypes

import numpy as np
import pytest
import torch

import embtab as et
import footprint as fp
import ragged_split_ref as rs
import weighted_ref as wr
from embtab import _lib
from embtab import update as upd
from embtab.tables import Dynamic, Static, fused_update_path
from test_gpu_adagrad import KINDS, ScatteredColumns, dev, host, same

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CHUNK, ROWS, ETA, HOT = rs.CHUNK, rs.ROWS, rs.ETA, rs.HOT - 1
_CASES = {}


def case(seed=1):
    """(L, values, colptr) of split_case(seed), built once; a test that edits them copies."""
    if seed not in _CASES:
        _CASES[seed] = rs.split_case(seed)
    return _CASES[seed]


def grad(kind, A, delta, values, colptr, weights=None):
    Rg = et.RaggedIndices(dev(values), dev(colptr))
    return et.SparseEmbeddingUpdate(A.lookup_type, kind.dev(delta), Rg,
                                    None if weights is None else dev(weights))


def dense(A):
    if isinstance(A, ScatteredColumns):
        return A.dense()
    return host(A.to_dense() if isinstance(A, et.SplitEmbedding) else A.data)


def short_columns(ent):
    return np.array(sorted(c for c, e in ent.items() if len(e) <= CHUNK))


# --- 1. Float32: every geometry, fused and unfused, with consequences (a), (b), (c) -------------

@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("static", [True, False])
@pytest.mark.parametrize("dim", [4, 128, 200, 520, 7])
def test_float32(dim, static, weighted):
    kind = KINDS["f32"]
    L, values, colptr = case()
    rng = np.random.default_rng(100 + dim)
    table = rng.standard_normal((ROWS, dim)).astype(np.float32)
    delta = rng.standard_normal((len(L), dim)).astype(np.float32)
    w = rs.case_weights(1, values, colptr, np.float32) if weighted else None
    lt = Static(dim) if static else Dynamic
    new = lambda: et.SimpleEmbedding(dev(table), lt)
    A = new()
    fused = fused_update_path(A)
    assert fused == (static and dim * 4 <= 512)
    et.update_(et.Descent(ETA), A, grad(kind, A, delta, values, colptr, w), split=True)
    got = host(A.data)
    ref = table.copy()
    ent, g_of = rs.ref_step(kind, ref, delta, values, colptr, w, fused=fused)
    assert same(got, ref)
    untouched = np.setdiff1d(np.arange(ROWS), sorted(g_of))
    assert len(untouched) > 500 and rs.LONELY - 1 in untouched
    assert same(got[untouched], table[untouched])
    # (a) the same tensors with split=False: equal on every column of at most 256 entries, and
    # different in the hot column (the chunked path ran)
    E = new()
    et.update_(et.Descent(ETA), E, grad(kind, E, delta, values, colptr, w))
    exact = host(E.data)
    short = short_columns(ent)
    assert len(short) >= 40 and same(got[short], exact[short])
    assert (got[HOT] != exact[HOT]).any()
    if not weighted:
        # (b) all-ones weights against no weights: the whole table
        O = new()
        et.update_(et.Descent(ETA), O, grad(kind, O, delta, values, colptr,
                                            np.ones(len(values), np.float32)), split=True)
        assert same(host(O.data), got)
    else:
        # (c) the expanded gradient, every covered entry its own bag, no weights
        Eg, covered = wr.expanded_gradient(delta, w, colptr, len(values))
        lo, hi = int(colptr[0]) - 1, int(colptr[-1]) - 1
        assert covered[lo:hi].all() and covered.sum() == hi - lo and lo == rs.HEAD
        own = np.arange(lo + 1, hi + 2, dtype=np.int64)
        X = new()
        et.update_(et.Descent(ETA), X, grad(kind, X, Eg[lo:hi], values, own), split=True)
        assert same(host(X.data), got)
    assert et.check_errors() == 0


# --- 2. element types ---------------------------------------------------------------------------

@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("static", [True, False])
@pytest.mark.parametrize("dim", [64, 7])
@pytest.mark.parametrize("name", ["f64", "f16", "bf16"])
def test_element_types(name, dim, static, weighted):
    kind = KINDS[name]
    L, values, colptr = case()
    rng = np.random.default_rng(200 + dim)
    table = kind.fromf(rng.standard_normal((ROWS, dim)))
    delta = kind.fromf(rng.standard_normal((len(L), dim)))
    w = rs.case_weights(1, values, colptr, kind.C) if weighted else None
    lt = Static(dim) if static else Dynamic
    A = et.SimpleEmbedding(kind.dev(table), lt)
    fused = fused_update_path(A)
    assert fused == static
    et.update_(et.Descent(ETA), A, grad(kind, A, delta, values, colptr, w), split=True)
    got = host(A.data)
    ref = table.copy()
    ent, g_of = rs.ref_step(kind, ref, delta, values, colptr, w, fused=fused)
    assert same(got, ref) and not same(got, table)
    # (a): for Float16 the exact twin sums in Float32 too (ET_FLAG_F16_FP32_ACC)
    E = et.SimpleEmbedding(kind.dev(table), lt)
    et.update_(et.Descent(ETA), E, grad(kind, E, delta, values, colptr, w), f16_fp32_acc=True)
    short = short_columns(ent)
    assert same(got[short], host(E.data)[short])
    assert et.check_errors() == 0


@pytest.mark.parametrize("name", ["f32", "f64", "f16", "bf16"])
def test_f64_alpha_through_a_two_table_call(name):
    """A multi-table call on the generic path (Dynamic, dim 7) evaluates w - eta*g in Float64
    with the unconverted eta, as the exact multi-table paths do."""
    kind = KINDS[name]
    L, values, colptr = case()
    rng = np.random.default_rng(250)
    hs = [kind.fromf(rng.standard_normal((ROWS, 7))) for _ in range(2)]
    deltas = [kind.fromf(rng.standard_normal((len(L), 7))) for _ in range(2)]
    ws = [rs.case_weights(1, values, colptr, kind.C), None]
    As = [et.SimpleEmbedding(kind.dev(h), Dynamic) for h in hs]
    eta = 0.1  # not representable: convert(T, eta) and eta differ
    et.update_(et.Descent(eta), As, [grad(kind, A, d, values, colptr, w)
                                     for A, d, w in zip(As, deltas, ws)], split=True)
    for A, h, d, w in zip(As, hs, deltas, ws):
        ref = h.copy()
        rs.ref_step(kind, ref, d, values, colptr, w, eta=eta, fused=False, f64_alpha=True)
        assert same(host(A.data), ref)
        if name != "f64":
            other = h.copy()
            rs.ref_step(kind, other, d, values, colptr, w, eta=eta, fused=False)
            assert not same(other, ref)  # the Float64 alpha is visible
    assert et.check_errors() == 0


# --- 3. storage ---------------------------------------------------------------------------------

@pytest.mark.parametrize("store", ["split64", "colptr_vec"])
def test_storage(store):
    kind = KINDS["f32"]
    L, values, colptr = case()
    rng = np.random.default_rng(300)
    dim = 128
    table = rng.standard_normal((ROWS, dim)).astype(np.float32)
    delta = rng.standard_normal((len(L), dim)).astype(np.float32)
    w = rs.case_weights(1, values, colptr, np.float32)
    if store == "split64":
        A = et.SplitEmbedding(dev(table), 64)
    else:
        A = ScatteredColumns(table, dim + 4, rng)
    et.update_(et.Descent(ETA), A, grad(kind, A, delta, values, colptr, w), split=True)
    ref = table.copy()
    rs.ref_step(kind, ref, delta, values, colptr, w, fused=fused_update_path(A))
    assert same(dense(A), ref) and not same(ref, table)
    assert et.check_errors() == 0


# --- 4. multi-table -----------------------------------------------------------------------------

@pytest.mark.parametrize("exact", [None, False])
def test_multi_table_mixed(oracle, exact):
    """A weighted table, an unweighted ragged one, a mean-pooled one and a fixed-pool unweighted
    one in one update_ over a Preallocation-strided gradient: the first three share one
    et_ragged_sgd_split call per (path, eltype) group, the last follows `exact`."""
    kind = KINDS["f32"]
    L, values, colptr = case()
    B = len(L)
    rng = np.random.default_rng(400)
    dims = [128, 16, 200, 64]
    lts = [Static(128), Static(16), Dynamic, Static(64)]
    hs = [rng.standard_normal((ROWS, d)).astype(np.float32) for d in dims]
    As = [et.SimpleEmbedding(dev(h), lt) for h, lt in zip(hs, lts)]
    w0 = rs.case_weights(1, values, colptr, np.float32)
    Imat = rng.integers(1, 60, (B, 5)).astype(np.int64)
    Imat[:, 0] = 7  # 300 occurrences: the fixed-pool split mode cuts this column
    ragged = lambda: et.RaggedIndices(dev(values), dev(colptr))
    Is = [et.WeightedIndices(ragged(), dev(w0)), ragged(),
          et.WeightedIndices(ragged(), mode="mean"), dev(Imat)]
    k = 3
    y, back = et.rrule(et.maplookup, et.PreallocationStrategy(k), As, Is)
    delta = rng.standard_normal(tuple(y.shape)).astype(np.float32)
    grads = back(dev(delta))[2]
    assert grads[0].delta.stride(0) == k + sum(dims)  # Preallocation-strided
    assert grads[0].weights is not None and grads[1].weights is None
    assert grads[2].weights is not None and grads[3].weights is None
    indexers = [et.Indexer() for _ in As]
    et.update_(et.Descent(ETA), As, grads, indexers, exact=exact, split=True)
    offs = np.cumsum([k] + dims)
    blk = [np.ascontiguousarray(delta[:, offs[t]:offs[t + 1]]) for t in range(4)]
    wmean = host(grads[2].weights)  # (d): mean mode carries w_k = 1 / len(bag(k))
    bag = np.repeat(np.arange(B), L)
    assert np.allclose(wmean[rs.HEAD:rs.HEAD + len(bag)], 1.0 / L[bag], rtol=1e-6, atol=0)
    for t, w in ((0, w0), (1, None), (2, wmean)):
        ref = hs[t].copy()
        # a multi-table call: Float64 alpha on the unfused path
        fused = fused_update_path(As[t])
        rs.ref_step(kind, ref, blk[t], values, colptr, w, fused=fused, f64_alpha=not fused)
        assert same(host(As[t].data), ref), t
    # the fixed-pool table: what update_ gives it alone with the same `exact`
    F = et.SimpleEmbedding(dev(hs[3]), lts[3])
    et.update_(et.Descent(ETA), [F], [et.SparseEmbeddingUpdate(F.lookup_type, dev(blk[3]),
                                                               dev(Imat))], exact=exact)
    assert same(host(As[3].data), host(F.data))
    ser = hs[3].copy()
    oracle.sgd(ser, blk[3], Imat, ETA, fused=True)
    assert same(host(F.data)[6], ser[6]) == (exact is None)  # it follows `exact`
    # Indexers are filled as on the exact path
    As2 = [et.SimpleEmbedding(dev(h), lt) for h, lt in zip(hs, lts)]
    indexers2 = [et.Indexer() for _ in As]
    et.update_(et.Descent(ETA), As2, grads, indexers2)
    for a, b in zip(indexers, indexers2):
        assert same(host(a.cumulative), host(b.cumulative)) and same(host(a.map), host(b.map))
        assert a.nunique == b.nunique > 0
    assert et.check_errors() == 0


def test_thirty_three_tables_make_two_calls(monkeypatch):
    kind = KINDS["f32"]
    rng = np.random.default_rng(410)
    n, R, dim, B = 33, 20, 4, 6
    hs, As, grads, parts = [], [], [], []
    for t in range(n):
        Lt = rng.integers(0, 5, B).astype(np.int64)
        v = rng.integers(1, R + 1, int(Lt.sum()) + 2).astype(np.int64)
        cp = wr.colptr_of(Lt)
        d = rng.standard_normal((B, dim)).astype(np.float32)
        w = rng.standard_normal(len(v)).astype(np.float32) if t % 2 else None
        hs.append(rng.standard_normal((R, dim)).astype(np.float32))
        As.append(et.SimpleEmbedding(dev(hs[-1]), Static(dim)))
        grads.append(grad(kind, As[-1], d, v, cp, w))
        parts.append((d, v, cp, w))
    calls = []
    real = upd._ragged_sgd_split
    monkeypatch.setattr(upd, "_ragged_sgd_split",
                        lambda descs, *a, **kw: (calls.append((len(descs), a[-1])),
                                                 real(descs, *a, **kw)))
    et.update_(et.Descent(ETA), As, grads, split=True)
    assert [c[0] for c in calls] == [32, 1]
    assert calls[0][1] != calls[1][1]  # a workspace key of its own
    for A, h, (d, v, cp, w) in zip(As, hs, parts):
        ref = h.copy()
        rs.ref_step(kind, ref, d, v, cp, w, fused=True)
        assert same(host(A.data), ref)
    assert et.check_errors() == 0


# --- 5. edges -----------------------------------------------------------------------------------

@pytest.mark.parametrize("dim", [128, 7])
def test_out_of_range_and_clamped_bounds_are_counted(dim):
    kind = KINDS["f32"]
    L, values, colptr = (a.copy() for a in case())
    rng = np.random.default_rng(500)
    nnz = len(values)
    used = np.arange(rs.HEAD, int(colptr[-1]) - 1)
    bad = rng.choice(used[values[used] < 400], 6, replace=False)
    values[bad[:3]], values[bad[3:]] = 0, ROWS + 1
    colptr[-1] = nnz + 50  # the last bag runs past the capacity: clamped to nnz, counted
    rg, clamped = wr.ranges(colptr, nnz)
    assert clamped == 1 and rg[-1][1] == nnz
    w = rs.case_weights(1, values, colptr, np.float32)
    assert not np.isnan(w[rs.HEAD:]).any()
    table = rng.standard_normal((ROWS, dim)).astype(np.float32)
    delta = rng.standard_normal((len(L), dim)).astype(np.float32)
    for weights in (w, None):
        A = et.SimpleEmbedding(dev(table))
        et.check_errors()
        et.update_(et.Descent(ETA), A, grad(kind, A, delta, values, colptr, weights), split=True)
        assert et.check_errors() == 6 + clamped
        ref = table.copy()
        _, g_of = rs.ref_step(kind, ref, delta, values, colptr, weights,
                              fused=fused_update_path(A))
        assert rs.LONELY - 1 in g_of  # the clamped last bag now covers the tail
        assert same(host(A.data), ref)


@pytest.mark.parametrize("dim", [16, 7])
def test_uncovered_entries_zero_weights_and_nan_by_position(dim):
    kind = KINDS["f32"]
    L, values, colptr = case()
    rng = np.random.default_rng(510)
    table = rng.standard_normal((ROWS, dim)).astype(np.float32)
    delta = rng.standard_normal((len(L), dim)).astype(np.float32)
    w = rs.case_weights(1, values, colptr, np.float32)
    lo, hi = int(colptr[0]) - 1, int(colptr[-1]) - 1
    assert np.isnan(w[:lo]).all() and np.isnan(w[hi:]).all()  # never read, never shown
    # a column whose every covered entry has weight 0 still participates: its 0 * Inf is NaN,
    # exactly where the Inf sits, and shows in the table
    zero_row = int(values[lo])
    w[lo:hi][values[lo:hi] == zero_row] = 0.0
    bag_of = np.zeros(len(values), np.int64)
    for j, (a, b) in enumerate(wr.ranges(colptr, len(values))[0]):
        bag_of[a:b] = j
    inf_bag = int(bag_of[lo])
    delta[inf_bag, 1] = np.inf
    A = et.SimpleEmbedding(dev(table), Static(dim))
    et.update_(et.Descent(ETA), A, grad(kind, A, delta, values, colptr, w), split=True)
    got = host(A.data)
    ref = table.copy()
    _, g_of = rs.ref_step(kind, ref, delta, values, colptr, w, fused=True)
    assert same(got, ref)
    assert zero_row - 1 in g_of and np.isnan(g_of[zero_row - 1][1])  # 0 * Inf
    assert np.isnan(got[zero_row - 1, 1]) and not np.isnan(got[zero_row - 1, 2:]).any()
    assert same(got[rs.LONELY - 1], table[rs.LONELY - 1])  # uncovered entries only
    assert not np.isnan(np.delete(got, zero_row - 1, axis=0)[:, [0] + list(range(2, dim))]).any()
    assert et.check_errors() == 0


def test_empty_gradients_are_no_ops_and_nontemporal_agrees():
    kind = KINDS["f32"]
    L, values, colptr = case()
    rng = np.random.default_rng(520)
    dim = 128
    table = rng.standard_normal((ROWS, dim)).astype(np.float32)
    A = et.SimpleEmbedding(dev(table))
    none = np.zeros(0, np.int64)
    for vals, cp, nb in ((none, np.ones(5, np.int64), 4), (none, np.ones(1, np.int64), 0),
                         (values, np.ones(1, np.int64), 0)):
        for w in (None, np.ones(len(vals), np.float32)):
            g = grad(kind, A, np.zeros((nb, dim), np.float32), vals, cp, w)
            et.update_(et.Descent(ETA), A, g, split=True)
            et.update_(et.Descent(ETA), [A], [g], split=True)
    assert same(host(A.data), table)
    delta = rng.standard_normal((len(L), dim)).astype(np.float32)
    w = rs.case_weights(1, values, colptr, np.float32)
    got = []
    for nt in (True, False):
        T = et.SimpleEmbedding(dev(table))
        et.update_(et.Descent(ETA), T, grad(kind, T, delta, values, colptr, w), split=True,
                   nontemporal=nt)
        got.append(host(T.data))
    assert same(got[0], got[1]) and not same(got[0], table)
    assert et.check_errors() == 0


# --- 6. memory ----------------------------------------------------------------------------------

@pytest.mark.parametrize("dim,left,ld", [(128, 8, 144), (7, 3, 13)])
def test_footprint(dim, left, ld):
    """A workspace of exactly the queried size poisoned with 0xFF, run twice: the same result
    both times; canaries around the table, the gradient (a view inside a larger NaN-filled
    buffer) and the weights stay; one byte less is ET_ERR_WORKSPACE and writes nothing."""
    kind = KINDS["f32"]
    L, values, colptr = case()
    rng = np.random.default_rng(600 + dim)
    table = rng.standard_normal((ROWS, dim)).astype(np.float32)
    delta = rng.standard_normal((len(L), dim)).astype(np.float32)
    w = rs.case_weights(1, values, colptr, np.float32)
    tbuf, tview, tintact = fp.guarded_matrix(ROWS, dim, torch.float32, DEV, left=left, ld=ld)
    big = torch.full((len(L) + 2, ld), float("nan"), device=DEV)
    dview = big[1:1 + len(L), left:left + dim]
    dview.copy_(dev(delta))
    dsnap = fp.snapshot(big)
    wbuf, wraw = fp.guarded_bytes(4 * len(values), 0, DEV)
    wraw.copy_(dev(w).view(torch.uint8))
    vals, cp = dev(values), dev(colptr)
    D = _lib.WeightedUpdateDesc
    descs = (D * 1)(D(tview.data_ptr(), ld, ROWS, dim, 0, dview.data_ptr(), ld, vals.data_ptr(),
                      len(values), cp.data_ptr(), len(L), 0, wraw.data_ptr(), None))
    Lb = _lib.load()
    nb = ctypes.c_int64(0)
    _lib.check(Lb.et_ragged_sgd_split_workspace_size(ctypes.addressof(descs), 1, ctypes.byref(nb)))
    ref = table.copy()
    rs.ref_step(kind, ref, delta, values, colptr, w, fused=True)

    def run(ptr, nbytes):
        return Lb.et_ragged_sgd_split(_lib.ET_F32, ctypes.addressof(descs), 1, ETA,
                                      _lib.ET_FLAG_NONTEMPORAL, ptr, nbytes, _lib.stream_handle())

    results = []
    for poison in (0xFF, 0xFF, 0x00):
        sbuf, ws = fp.guarded_bytes(nb.value, 0, DEV)
        ws.fill_(poison)
        tview.copy_(dev(table))
        _lib.check(run(ws.data_ptr(), nb.value))
        torch.cuda.synchronize()
        fp.assert_guards(sbuf, ws, "workspace")
        results.append(host(tview))
        assert same(results[-1], ref)
    assert same(results[0], results[1]) and same(results[0], results[2])
    ok, where = tintact()
    assert ok, where
    fp.assert_guards(wbuf, wraw, "weights")
    assert fp.unchanged(big, dsnap)
    # one byte short (both alignments of the 256-byte slack): refused, nothing written
    for shift in (0, 1):
        need = nb.value - 256 + (256 - shift) % 256
        sbuf, ws = fp.guarded_bytes(nb.value, shift, DEV)
        ws.fill_(0xFF)
        tview.copy_(dev(table))
        assert run(ws.data_ptr(), need - 1) == -3
        torch.cuda.synchronize()
        assert b"%d bytes" % need in Lb.et_last_error()
        fp.assert_guards(sbuf, ws, "short workspace")
        assert bool((ws == 0xFF).all()) and same(host(tview), table)
    assert et.check_errors() == 0


# --- 7. graph capture ---------------------------------------------------------------------------

def test_graph_capture_refill():
    kind = KINDS["f32"]
    dim, CAP = 128, 8000
    rng = np.random.default_rng(700)
    table = rng.standard_normal((ROWS, dim)).astype(np.float32)
    L1, v1, cp1 = case(1)
    L2, v2, cp2 = rs.split_case(2, tail=140)  # another total length
    assert len(v1) != len(v2) and max(len(v1), len(v2)) <= CAP and len(L1) == len(L2)
    vals = torch.ones(CAP, dtype=torch.int64, device=DEV)
    wts = torch.full((CAP,), float("nan"), device=DEV)
    colptr = torch.ones(len(L1) + 1, dtype=torch.int64, device=DEV)
    ddev = torch.zeros((len(L1), dim), device=DEV)
    Rg = et.RaggedIndices(vals, colptr)

    def fill(seed, v, cp):
        delta = np.random.default_rng(seed).standard_normal((len(L1), dim)).astype(np.float32)
        w = rs.case_weights(seed, v, cp, np.float32)
        vals.fill_(1)
        wts.fill_(float("nan"))
        vals[:len(v)].copy_(dev(v))
        wts[:len(w)].copy_(dev(w))
        colptr.copy_(dev(cp))
        ddev.copy_(dev(delta))
        return delta

    def step(T):
        et.update_(et.Descent(ETA), T, et.SparseEmbeddingUpdate(T.lookup_type, ddev, Rg, wts),
                   split=True)

    fill(1, v1, cp1)
    A = et.SimpleEmbedding(dev(table), Static(dim))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # one eager step first, on a scratch table
        step(et.SimpleEmbedding(dev(table), Static(dim)))
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step(A)
    delta2 = fill(2, v2, cp2)  # refill idx, colptr, weights and delta in place, then replay
    g.replay()
    torch.cuda.synchronize()
    ref = table.copy()
    rs.ref_step(kind, ref, delta2, host(vals), host(colptr), host(wts), fused=True)
    assert same(host(A.data), ref) and not same(ref, table)
    assert et.check_errors() == 0


# --- 8. thresholds: the second iteration of every capped grid-stride loop ---------------------------
#
# With n the call's entries, sgd_grid(n) = clamp(cdiv(n, 2048), 256, 16384) and GPW the lane
# groups per wave (64 / (D / 4) below capacity 256, else 1), one sweep covers
#   k_ragged_sgd_chunks<D>          sgd_grid(n) x 4 x GPW chunk records: 16,384 at capacity 16
#   k_ragged_sgd_chunks_generic     sgd_grid(n) x 4 = 1,024 chunk records (n <= 524,288)
#   k_ragged_sgd_combine<D>         min(cdiv(n / 256 + 2, 4 GPW), 2,048) x 4 x GPW multi-chunk
#                                   columns: the cap binds from 8,192 columns at capacity 256 and
#                                   above (131,072 at capacity 16: 33.7 M entries, not run)
#   k_ragged_sgd_combine_generic    min(cdiv(n / 256 + 2, 4), 4,096) x 4 = 16,384 columns
# Each case runs just past one of them and is compared with the model on sampled columns and
# with an eager run of the same data cut into two calls over disjoint halves of the columns.

def equal_count_case(ncols, count, R, B, dim, seed):
    rng = np.random.default_rng(seed)
    cols = 1 + np.sort(rng.choice(R, ncols, replace=False))
    values = rng.permutation(np.repeat(cols, count)).astype(np.int64)
    n = len(values)
    L = np.full(B, n // B, np.int64)
    L[:n % B] += 1
    table = rng.standard_normal((R, dim)).astype(np.float32)
    delta = rng.standard_normal((B, dim)).astype(np.float32)
    w = (0.25 + 1.75 * rng.random(n)).astype(np.float32)
    return cols, values, wr.colptr_of(L), table, delta, w


def sampled_model(kind, table, delta, values, colptr, w, cols, fused):
    """The model on the columns `cols` (1-based) alone; every entry is covered here, so a
    column's list is its entries in increasing k with their bags."""
    assert colptr[0] == 1 and colptr[-1] == len(values) + 1
    g_of = {}
    for c in cols:
        ks = np.nonzero(values == c)[0]
        bags = np.searchsorted(colptr - 1, ks, side="right")
        g_of[int(c) - 1] = rs.chunked_g(delta, list(zip(bags.tolist(), ks.tolist())), w)
    return rs.apply(kind, table.copy(), g_of, fused=fused)


@pytest.mark.parametrize("what,dim,ncols,count", [
    ("chunks<16>", 16, 16500, 2),          # 16,500 chunk records > 16,384
    ("chunks_generic", 7, 1100, 3),        # 1,100 > 1,024
    ("combine<256>", 256, 8200, 257),      # 8,200 multi-chunk columns > 8,192
    ("combine_generic", 1, 16400, 257),    # 16,400 > 16,384
])
def test_second_sweep(what, dim, ncols, count):
    kind = KINDS["f32"]
    R, B = ncols + 100, 4096
    cols, values, colptr, table, delta, w = equal_count_case(ncols, count, R, B, dim, 800 + dim)
    n = len(values)
    cap = None if dim % 4 else max(16, 1 << (dim - 1).bit_length())
    if what.startswith("chunks"):
        records = ncols * -(-count // CHUNK)
        assert records > rs.chunk_sweep(n, cap) and n <= 524288
    else:
        assert count > CHUNK and ncols > rs.combine_sweep(n, cap)
    A = et.SimpleEmbedding(dev(table), Static(dim))
    fused = fused_update_path(A)
    et.update_(et.Descent(ETA), A, grad(kind, A, delta, values, colptr, w), split=True)
    got = host(A.data)
    # the model on the first, the middle and the last columns of the sweep order
    sample = np.concatenate([cols[:3], cols[ncols // 2:ncols // 2 + 2], cols[-3:]])
    ref = sampled_model(kind, table, delta, values, colptr, w, sample, fused)
    assert same(got[sample - 1], ref[sample - 1])
    # an eager run of the same data cut into two calls: each half's sweep is a first one
    T = et.SimpleEmbedding(dev(table), Static(dim))
    half = cols[ncols // 2]
    et.check_errors()
    for keep in (values < half, values >= half):
        et.update_(et.Descent(ETA), T, grad(kind, T, delta, np.where(keep, values, 0), colptr, w),
                   split=True)
    assert et.check_errors() == n
    assert same(got, host(T.data))
    assert not (got[cols - 1] == table[cols - 1]).all(axis=1).any()  # every column was written
    untouched = np.setdiff1d(np.arange(R), cols - 1)
    assert same(got[untouched], table[untouched])
