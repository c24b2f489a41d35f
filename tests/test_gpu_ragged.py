"""Variable-length bags on the GPU: ragged lookup, fused ragged maplookup, the ragged sparse
SGD and the Indexer of ragged indices, all bit for bit against the existing oracle.

Expected values: a ragged lookup is a set of fixed-pool lookups grouped by bag length
(``oracle.pooled_sum`` on the ``(n_L, L)`` matrix of the bags of length ``L``; zeros for
``L == 0``); a ragged update is a vector-index update of the expanded gradient
(``oracle.sgd(table, delta[bag], values, ...)`` — the same entries in the same order).
Comparisons are ``tobytes()`` equality throughout."""
import numpy as np
import pytest
import torch

import embtab as et
from embtab.tables import AbstractEmbeddingTable, Dynamic, Static, fused_update_path

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROWS = 700
# every length at which the vector kernel takes another path: U-1, U, U+1 for its U = 8
# (16-byte to 512-byte rows), 4 (2 KiB rows), 2 and 1 (longer rows), a bag longer than one
# index chunk of every geometry (33 > 32 lanes; 300 > 64 lanes), and empty bags
LENMIX = [0, 1, 2, 3, 4, 5, 7, 8, 9, 33, 300]


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def host(x):
    if x.dtype in (torch.bfloat16, torch.float16):
        return x.view(torch.int16).cpu().numpy().view(np.uint16 if x.dtype == torch.bfloat16
                                                      else np.float16)
    return x.cpu().numpy()


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def mix_lengths(B, rng, extra=()):
    """First and last bag empty, every LENMIX length (and `extra`) at least once."""
    must = LENMIX + list(extra)
    assert B >= len(must) + 2
    L = rng.integers(0, 13, B)
    pos = 1 + rng.permutation(B - 2)[:len(must)]
    L[pos] = must
    L[0] = L[-1] = 0
    return L.astype(np.int64)


def colptr_of(L):
    return np.concatenate([[1], 1 + np.cumsum(L)]).astype(np.int64)


def ranges_of(colptr, nnz):
    """The kernels' clamping rule: 0 <= lo <= hi <= nnz."""
    out = []
    for j in range(len(colptr) - 1):
        lo = min(max(int(colptr[j]) - 1, 0), nnz)
        hi = min(max(int(colptr[j + 1]) - 1, lo), nnz)
        out.append((lo, hi))
    return out


def expect_lookup(oracle, table, values, ranges, **kw):
    """Fixed-pool oracle lookups grouped by bag length."""
    out = np.zeros((len(ranges), table.shape[1]), table.dtype)
    lens = np.array([hi - lo for lo, hi in ranges])
    for L in np.unique(lens):
        if L == 0:
            continue
        sel = np.nonzero(lens == L)[0]
        I = np.stack([values[ranges[j][0]:ranges[j][1]] for j in sel])
        out[sel] = oracle.pooled_sum(table, I, **kw)
    return out


def ragged(values, colptr):
    return et.RaggedIndices(dev(values), dev(colptr))


@pytest.fixture(scope="module")
def mix301():
    rng = np.random.default_rng(301)
    L = mix_lengths(301, rng)
    return L, rng.integers(1, ROWS + 1, int(L.sum())).astype(np.int64)


# --- 1. forward geometry ---------------------------------------------------------------------

@pytest.mark.parametrize("dim", [16, 128, 512, 1504, 20, 7])
def test_forward_geometry(oracle, mix301, dim):
    L, values = mix301
    rng = np.random.default_rng(dim)
    table = rng.standard_normal((ROWS, dim)).astype(np.float32)
    A = et.SimpleEmbedding(dev(table))
    R = ragged(values, colptr_of(L))
    want = expect_lookup(oracle, table, values, ranges_of(colptr_of(L), len(values)))
    assert same(host(et.lookup(A, R)), want)
    assert et.destination(A, R).shape == (301, dim)
    assert same(host(et.lookup_(et.destination(A, R), A, R, nontemporal=False)), want)
    # a strided destination: columns 4 .. 4+D of a wider tensor, surroundings untouched
    wide = torch.full((301, dim + 9), -3.0, device=DEV)
    et.lookup_(wide[:, 4:4 + dim], A, R)
    w = host(wide)
    assert same(w[:, 4:4 + dim], want)
    assert (w[:, :4] == -3).all() and (w[:, 4 + dim:] == -3).all()
    # every bag empty (no entry at all, then unused capacity); a single bag
    for cap in (0, 5):
        E = ragged(values[:cap], np.ones(302, np.int64))
        assert same(host(et.lookup(A, E)), np.zeros((301, dim), np.float32))
    one = ragged(values[:11], np.array([1, 12], np.int64))
    assert same(host(et.lookup(A, one)), oracle.pooled_sum(table, values[None, :11]))
    assert et.check_errors() == 0


# --- 2. signed zeros: the first row is copied, an empty bag is +0 ----------------------------

@pytest.mark.parametrize("dim", [16, 7])
def test_signed_zeros_and_copy_first(oracle, dim):
    table = np.random.default_rng(2).standard_normal((ROWS, dim)).astype(np.float32)
    table[[4, 9]] = -0.0
    #        [-0]  [-0, -0]  []  [-0, x]  [x, -0]  [x]
    L = np.array([1, 2, 0, 2, 2, 1])
    values = np.array([5, 5, 10, 10, 3, 3, 5, 7], np.int64)
    got = host(et.lookup(et.SimpleEmbedding(dev(table)), ragged(values, colptr_of(L))))
    want = expect_lookup(oracle, table, values, ranges_of(colptr_of(L), len(values)))
    assert same(got, want)
    sign = np.signbit(got)
    assert sign[0].all() and sign[1].all() and not sign[2].any()  # -0, -0 + -0 = -0, +0


# --- 3. element types ----------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["f64", "f16", "f16acc", "bf16", "i32", "i64"])
def test_forward_element_types(oracle, kind):
    from oracle import f32_to_bf16

    rng = np.random.default_rng(3)
    B, D = 130, 64
    L = mix_lengths(B, rng)
    values = rng.integers(1, ROWS + 1, int(L.sum())).astype(np.int64)
    x = rng.standard_normal((ROWS, D))
    kw = {}
    if kind == "bf16":
        table, tdev, kw = f32_to_bf16(x.astype(np.float32)), None, {"bf16": True}
        tdev = dev(table.view(np.int16)).view(torch.bfloat16)
    elif kind in ("i32", "i64"):
        table = rng.integers(-2**20, 2**20, (ROWS, D)).astype(np.int32 if kind == "i32"
                                                              else np.int64)
        tdev = dev(table)
    else:
        table = x.astype({"f64": np.float64}.get(kind, np.float16))
        tdev = dev(table)
        if kind == "f16acc":
            kw = {"f16_fp32_acc": True}
    A = et.SimpleEmbedding(tdev)
    R = ragged(values, colptr_of(L))
    want = expect_lookup(oracle, table, values, ranges_of(colptr_of(L), len(values)), **kw)
    dst = torch.empty((B, D), dtype=tdev.dtype, device=DEV)
    et.maplookup_(et.PreallocationStrategy(0), dst, [A], [R], f16_fp32_acc=kind == "f16acc")
    assert same(host(dst), want)
    if kind != "f16acc":
        assert same(host(et.lookup(A, R)), want)
    assert et.check_errors() == 0


# --- 4. storage: paged and column-pointer-only tables ----------------------------------------

class ScatteredColumns(AbstractEmbeddingTable):
    """Columns at permuted slots of a pool: only ``columnpointer`` describes the layout."""

    def __init__(self, cols, pitch, rng, lookup_type=Dynamic):
        self.R, self.D = cols.shape
        self.perm = rng.permutation(self.R)
        pool = np.zeros((self.R, pitch), cols.dtype)
        pool[self.perm, :self.D] = cols
        self.pool, self.pitch, self.lookup_type = dev(pool.reshape(-1)), pitch, lookup_type

    def size(self):
        return (self.D, self.R)

    def columnpointer(self, i, ctx=None):
        return self.pool.data_ptr() + int(self.perm[i - 1]) * self.pitch * 4

    def example(self):
        return self.pool[:self.D].view(1, self.D)

    def dense(self):
        return host(self.pool).reshape(self.R, self.pitch)[self.perm, :self.D]


@pytest.mark.parametrize("store", ["split64", "colptr_vec", "colptr_generic"])
def test_storage_forward_and_update(oracle, store):
    rng = np.random.default_rng(4)
    B = 130
    D = 128 if store != "colptr_generic" else 10
    L = mix_lengths(B, rng)
    values = rng.integers(1, ROWS + 1, int(L.sum())).astype(np.int64)
    table = rng.standard_normal((ROWS, D)).astype(np.float32)
    if store == "split64":
        A = et.SplitEmbedding(dev(table), 64)
        dense = lambda: host(A.to_dense())
    else:
        A = ScatteredColumns(table, D + (4 if store == "colptr_vec" else 3), rng)
        dense = A.dense
    R = ragged(values, colptr_of(L))
    want = expect_lookup(oracle, table, values, ranges_of(colptr_of(L), len(values)))
    assert same(host(et.lookup(A, R)), want)
    delta = rng.standard_normal((B, D)).astype(np.float32)
    et.update_(et.Descent(0.1), A, et.SparseEmbeddingUpdate(A.lookup_type, dev(delta), R))
    bag = np.repeat(np.arange(B), L)
    oracle.sgd(table, delta[bag], values, 0.1, fused=fused_update_path(A))
    assert same(dense(), table)
    assert et.check_errors() == 0


# --- 5. fused concat --------------------------------------------------------------------------

@pytest.mark.parametrize("k", [0, 16])
def test_fused_concat_mixed_indices(oracle, k):
    rng = np.random.default_rng(5)
    B, dims = 140, [16, 128, 20]
    tables = [rng.standard_normal((ROWS, d)).astype(np.float32) for d in dims]
    As = [et.SimpleEmbedding(dev(t)) for t in tables]
    L = mix_lengths(B, rng)
    values = rng.integers(1, ROWS + 1, int(L.sum())).astype(np.int64)
    Imat = rng.integers(1, ROWS + 1, (B, 12)).astype(np.int64)
    Ivec = rng.integers(1, ROWS + 1, B).astype(np.int64)
    R = ragged(values, colptr_of(L))
    Is = [R, dev(Imat), dev(Ivec)]

    def pieces(vals):
        return [expect_lookup(oracle, tables[0], vals, ranges_of(colptr_of(L), len(vals))),
                oracle.pooled_sum(tables[1], Imat), oracle.gather(tables[2], Ivec)]

    want = np.concatenate(pieces(values), axis=1)
    strat = et.PreallocationStrategy(k)
    dst = torch.full((B, k + sum(dims)), -3.0, device=DEV)
    et.maplookup_(strat, dst, As, Is)
    got = host(dst)
    assert same(got[:, k:], want)
    assert (got[:, :k] == -3).all()  # the prepended columns are not touched
    assert same(host(et.maplookup(strat, As, Is))[:, k:], want)
    per_table = [host(et.lookup(A, i)) for A, i in zip(As, Is)]
    assert same(np.concatenate(per_table, axis=1), want)
    for y, w in zip(et.maplookup(et.DefaultStrategy(), As, Is), pieces(values)):
        assert same(host(y), w)
    for y, w in zip(et.maplookup(et.SimpleParallelStrategy(), As, Is), pieces(values)):
        assert same(host(y), w)
    # a plan: descriptors built once, the values refilled in place between two calls
    plan = et.PreallocationPlan(strat, dst, As, Is)
    assert same(host(plan())[:, k:], want)
    values2 = rng.integers(1, ROWS + 1, len(values)).astype(np.int64)
    R.values.copy_(dev(values2))
    assert same(host(plan())[:, k:], np.concatenate(pieces(values2), axis=1))
    # a strided (B, P) matrix cannot be described by an arithmetic colptr
    wide = dev(rng.integers(1, ROWS + 1, (B, 16)).astype(np.int64))
    with pytest.raises(NotImplementedError, match="table 1"):
        et.maplookup_(strat, dst, As, [R, wide[:, :12], Is[2]])
    assert et.check_errors() == 0


# --- 6. clamping, without risk -----------------------------------------------------------------

def test_clamping_reads_only_owned_memory(oracle):
    rng = np.random.default_rng(6)
    D, B, CAP = 128, 40, 500
    table = rng.standard_normal((ROWS, D)).astype(np.float32)
    A = et.SimpleEmbedding(dev(table))
    # `values` is a view of the first 500 entries of a 2000-entry buffer of valid indices:
    # even a kernel that forgot to clamp would read only memory this test owns
    buf = rng.integers(1, ROWS + 1, 2000).astype(np.int64)
    dbuf = dev(buf)
    L = rng.integers(5, 13, B)
    colptr = colptr_of(L)
    assert colptr[-1] - 1 <= CAP
    colptr[-1] = 900                 # claims 400 entries beyond the capacity
    colptr[18] = colptr[17] - 3      # an interior pair decreases
    et.check_errors()
    R = et.RaggedIndices(dbuf[:CAP], dev(colptr))
    got = host(et.lookup(A, R))
    assert et.check_errors() == 2    # bag 17's hi (raised to its lo), the last bag's hi
    rg = ranges_of(colptr, CAP)
    assert rg[17][0] == rg[17][1] and rg[-1][1] == CAP and rg[18][0] == colptr[17] - 4
    want = expect_lookup(oracle, table, buf[:CAP], rg)
    assert same(got, want)
    clean = [j for j in range(B) if j not in (17, 18, B - 1)]
    exact = expect_lookup(oracle, table, buf, ranges_of(colptr_of(L), 2000))
    assert same(got[clean], exact[clean])
    # the generic kernel clamps the same way
    A7 = et.SimpleEmbedding(dev(table[:, :7]))
    got7 = host(et.lookup(A7, R))
    assert et.check_errors() == 2
    assert same(got7, expect_lookup(oracle, np.ascontiguousarray(table[:, :7]), buf[:CAP], rg))
    # an index outside 1..nrows is counted and contributes a zero row
    vals = buf[:CAP].copy()
    vals[[3, 77]] = [0, ROWS + 1]
    zrow = np.concatenate([table, np.zeros((1, D), np.float32)])
    as_zero = np.where((vals < 1) | (vals > ROWS), ROWS + 1, vals)
    ok_colptr = colptr_of(L)
    for AA, tt in ((A, zrow), (A7, np.ascontiguousarray(zrow[:, :7]))):
        got = host(et.lookup(AA, ragged(vals, ok_colptr)))
        assert et.check_errors() == 2
        assert same(got, expect_lookup(oracle, tt, as_zero, ranges_of(ok_colptr, CAP)))


# --- 7. update, single table --------------------------------------------------------------------

def hot_case(B, rng, nrows=ROWS):
    """The length mix plus ten bags of 300 entries of one hot row (3,000 entries: one serial
    column well past ET_SGD_CHUNK); the other values from 40 distinct rows."""
    L = mix_lengths(B, rng, extra=[300] * 10)
    cp = colptr_of(L)
    rows40 = rng.choice(nrows, 40, replace=False) + 1
    values = rows40[rng.integers(1, 40, int(L.sum()))].astype(np.int64)
    hot = np.nonzero(L == 300)[0][1:]
    assert len(hot) == 10
    for j in hot:
        values[cp[j] - 1:cp[j + 1] - 1] = rows40[0]
    return L, values, rows40


@pytest.mark.parametrize("dim,static", [(16, True), (16, False), (128, True), (128, False),
                                        (200, False), (1504, False)])
def test_update_single_table(oracle, dim, static):
    rng = np.random.default_rng(7 + dim)
    B = 257
    L, values, rows40 = hot_case(B, rng)
    assert (values == rows40[0]).sum() >= 3000 > et._lib.ET_SGD_CHUNK
    table = rng.standard_normal((ROWS, dim)).astype(np.float32)
    delta = rng.standard_normal((B, dim)).astype(np.float32)
    bag = np.repeat(np.arange(B), L)
    lt = Static(dim) if static else Dynamic
    fused = static and dim * 4 <= 512
    ref = table.copy()
    oracle.sgd(ref, delta[bag], values, 0.1, fused=fused)
    untouched = np.setdiff1d(np.arange(ROWS), values - 1)
    assert len(untouched) > 600 and same(ref[untouched], table[untouched])

    A = et.SimpleEmbedding(dev(table), lt)
    assert fused_update_path(A) == fused
    R = ragged(values, colptr_of(L))
    et.update_(et.Descent(0.1), A, et.SparseEmbeddingUpdate(lt, dev(delta), R))
    assert same(host(A.data), ref)
    # exact=False is accepted and exact anyway; delta as a strided view
    A = et.SimpleEmbedding(dev(table), lt)
    wide = torch.zeros((B, dim + 8), device=DEV)
    wide[:, 4:4 + dim] = dev(delta)
    et.update_(et.Descent(0.1), A, et.SparseEmbeddingUpdate(lt, wide[:, 4:4 + dim], R),
               exact=False, nontemporal=False)
    assert same(host(A.data), ref)
    # a capacity tail of valid indices of otherwise unreferenced rows changes nothing
    A = et.SimpleEmbedding(dev(table), lt)
    tail = (untouched[:50] + 1).astype(np.int64)
    Rt = ragged(np.concatenate([values, tail]), colptr_of(L))
    assert Rt.nnz == len(values) + 50
    et.update_(et.Descent(0.1), A, et.SparseEmbeddingUpdate(lt, dev(delta), Rt))
    assert same(host(A.data), ref)
    # an empty gradient (no entries; then no entry in use) leaves the table unchanged
    A = et.SimpleEmbedding(dev(table), lt)
    for E in (ragged(values[:0], np.ones(B + 1, np.int64)),
              ragged(values[:9], np.ones(B + 1, np.int64))):
        et.update_(et.Descent(0.1), A, et.SparseEmbeddingUpdate(lt, dev(delta), E))
        assert same(host(A.data), table)
    assert et.check_errors() == 0


# --- 8. update, element types --------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["f64", "f16", "f16acc", "bf16"])
@pytest.mark.parametrize("static", [True, False])
def test_update_element_types(oracle, kind, static):
    from oracle import f32_to_bf16

    rng = np.random.default_rng(8)
    B, D = 130, 64
    L, values, _ = hot_case(B, rng)
    x = rng.standard_normal((ROWS, D)).astype(np.float32)
    d = (0.05 * rng.standard_normal((B, D))).astype(np.float32)
    if kind == "bf16":
        base, delta = f32_to_bf16(x), f32_to_bf16(d)
        tdev = dev(base.view(np.int16)).view(torch.bfloat16)
        ddev = dev(delta.view(np.int16)).view(torch.bfloat16)
    else:
        dt = np.float64 if kind == "f64" else np.float16
        base, delta = x.astype(dt), d.astype(dt)
        tdev, ddev = dev(base), dev(delta)
    lt = Static(D) if static else Dynamic
    A = et.SimpleEmbedding(tdev, lt)
    et.update_(et.Descent(0.1), A, et.SparseEmbeddingUpdate(lt, ddev, ragged(values,
                                                                             colptr_of(L))),
               f16_fp32_acc=kind == "f16acc")
    ref = base.copy()
    oracle.sgd(ref, delta[np.repeat(np.arange(B), L)], values, 0.1, fused=fused_update_path(A),
               bf16=kind == "bf16", f16_fp32_acc=kind == "f16acc")
    assert same(host(A.data), ref)
    assert et.check_errors() == 0


# --- 9. update, multi-table ------------------------------------------------------------------------

@pytest.mark.parametrize("k", [0, 3])
def test_update_multi_table_mixed(oracle, k):
    rng = np.random.default_rng(9)
    B, dims = 140, [16, 128, 64, 200]
    lts = [Static(16), Dynamic, Static(64), Dynamic]
    hs = [rng.standard_normal((ROWS, d)).astype(np.float32) for d in dims]
    As = [et.SimpleEmbedding(dev(h), lt) for h, lt in zip(hs, lts)]
    La, Lb = mix_lengths(B, rng), mix_lengths(B, rng)
    va = rng.integers(1, 60, int(La.sum())).astype(np.int64)
    vb = rng.integers(1, 60, int(Lb.sum())).astype(np.int64)
    Imat = rng.integers(1, 60, (B, 5)).astype(np.int64)
    Ivec = rng.integers(1, 60, B).astype(np.int64)
    Ra, Rb = ragged(va, colptr_of(La)), ragged(vb, colptr_of(Lb))
    Is = [Ra, dev(Imat), Rb, dev(Ivec)]  # ragged, fixed-pool, ragged, vector
    strat = et.PreallocationStrategy(k)
    y, back = et.rrule(et.maplookup, strat, As, Is)
    delta = rng.standard_normal(tuple(y.shape)).astype(np.float32)
    grads = back(dev(delta))[2]
    assert grads[0].indices is Ra and grads[2].indices is Rb
    assert grads[1].delta.stride(0) == k + sum(dims)  # Preallocation-strided gradients
    indexers = [et.Indexer() for _ in As]
    et.update_(et.Descent(0.1), As, grads, indexers)
    offs = np.cumsum([k] + dims)
    bags = [np.repeat(np.arange(B), La), None, np.repeat(np.arange(B), Lb), None]
    exp_d, exp_i = [], []
    for t, (b, I) in enumerate(zip(bags, [va, Imat, vb, Ivec])):
        blk = np.ascontiguousarray(delta[:, offs[t]:offs[t + 1]])
        exp_d.append(blk if b is None else blk[b])
        exp_i.append(I)
    oracle.sgd_multi(hs, exp_d, exp_i, 0.1, [fused_update_path(A) for A in As])
    for A, h in zip(As, hs):
        assert same(host(A.data), h)
    for t, b in enumerate(bags):
        cum, mp = oracle.index_build(exp_i[t], ROWS)
        if b is not None:
            mp = b[mp - 1] + 1  # entry -> its bag, the gradient column
        assert same(host(indexers[t].cumulative), cum)
        assert same(host(indexers[t].map), mp)
    with pytest.raises(NotImplementedError):
        et.PhasedUpdate(As, grads)
    assert et.check_errors() == 0


# --- 10. two independent paths agree ------------------------------------------------------------

@pytest.mark.parametrize("static", [True, False])
def test_fused_update_equals_indexer_views(oracle, static):
    rng = np.random.default_rng(10)
    B, D = 130, 128
    L, values, _ = hot_case(B, rng)
    table = rng.standard_normal((ROWS, D)).astype(np.float32)
    delta = rng.standard_normal((B, D)).astype(np.float32)
    lt = Static(D) if static else Dynamic
    # a capacity tail: the Indexer covers the used entries only
    R = ragged(np.concatenate([values, values[:7]]), colptr_of(L))
    A1, A2 = et.SimpleEmbedding(dev(table), lt), et.SimpleEmbedding(dev(table), lt)
    g = et.SparseEmbeddingUpdate(lt, dev(delta), R)
    et.update_(et.Descent(0.1), A1, g)
    ix = et.index_(et.Indexer(), R, ROWS)
    assert int(ix.map.numel()) == len(values)
    for split in range(1, 5):
        et.update_(A2, g, et.IndexerView(ix, 4, split), 0.1)
    ref = table.copy()
    oracle.sgd(ref, delta[np.repeat(np.arange(B), L)], values, 0.1, fused=fused_update_path(A1))
    assert same(host(A1.data), host(A2.data))
    assert same(host(A1.data), ref)
    assert et.check_errors() == 0


# --- 11. rrule and uncompress --------------------------------------------------------------------

def test_rrule_and_uncompress(oracle):
    rng = np.random.default_rng(11)
    B, D = 130, 32
    L = mix_lengths(B, rng)
    values = rng.integers(1, ROWS + 1, int(L.sum())).astype(np.int64)
    table = rng.standard_normal((ROWS, D)).astype(np.float32)
    A = et.SimpleEmbedding(dev(table), Static(D))
    R = ragged(np.concatenate([values, values[:5]]), colptr_of(L))  # with a capacity tail
    y, back = et.rrule(et.lookup, A, R)
    assert same(host(y), host(et.lookup(A, R)))
    delta = dev(rng.integers(-8, 9, (B, D)).astype(np.float32))  # small integers: exact sums
    _, grad, _ = back(delta)
    assert isinstance(grad, et.SparseEmbeddingUpdate) and grad.indices is R
    assert "RaggedIndices" in repr(grad)
    bag = torch.from_numpy(np.repeat(np.arange(B), L)).to(DEV)
    want = torch.zeros((ROWS, D), device=DEV)
    want.index_add_(0, dev(values) - 1, delta[bag])
    assert same(host(et.uncompress(grad, ROWS)), host(want))
    assert et.uncompress(grad).shape[0] == int(values.max())


# --- 12. graph capture: refill values / colptr in place, replay another total ------------------

def test_graph_capture_refill(oracle):
    rng = np.random.default_rng(12)
    B, D, CAP = 130, 128, 3000
    table = rng.standard_normal((ROWS, D)).astype(np.float32)
    delta = rng.standard_normal((B, D)).astype(np.float32)

    def inputs(total_hint):
        L = mix_lengths(B, rng) if total_hint else rng.integers(0, 6, B).astype(np.int64)
        v = rng.integers(1, ROWS + 1, int(L.sum())).astype(np.int64)
        assert len(v) <= CAP
        return L, v

    L1, v1 = inputs(True)
    vals = torch.ones(CAP, dtype=torch.int64, device=DEV)
    colptr = torch.ones(B + 1, dtype=torch.int64, device=DEV)
    R = et.RaggedIndices(vals, colptr)
    ddev = dev(delta)
    A = et.SimpleEmbedding(dev(table), Static(D))
    dst = torch.empty((B, D), device=DEV)

    def fill(L, v):
        vals[:len(v)].copy_(dev(v))
        colptr.copy_(dev(colptr_of(L)))

    def step(T, out):
        et.lookup_(out, T, R)
        et.update_(et.Descent(0.1), T, et.SparseEmbeddingUpdate(T.lookup_type, ddev, R))

    fill(L1, v1)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # one eager step first (workspaces), on a scratch table
        step(et.SimpleEmbedding(dev(table), Static(D)), torch.empty_like(dst))
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step(A, dst)
    # another length mix with a smaller total (stale entries stay behind it), then replay
    L2, v2 = inputs(False)
    assert 0 < len(v2) < len(v1)
    fill(L2, v2)
    g.replay()
    torch.cuda.synchronize()
    assert same(host(dst), expect_lookup(oracle, table, v2, ranges_of(colptr_of(L2), CAP)))
    ref = table.copy()
    oracle.sgd(ref, delta[np.repeat(np.arange(B), L2)], v2, 0.1, fused=True)
    assert same(host(A.data), ref)
    assert et.check_errors() == 0
