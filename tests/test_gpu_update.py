"""Parity of the HIP sparse-SGD path and device Indexer with the oracle.

Mirrors test/update.jl (pullback structure, Descent update vs the dense update,
partition exactness), test/map.jl:117-177 (gradients through maplookup and
PreallocationStrategy) and test/misc.jl:74-110 (Indexer KAT)."""
import numpy as np
import pytest
import torch

import embtab as et

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CHUNK = et._lib.ET_SGD_CHUNK  # occurrences per chunk of the non-exact update


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def host(x):
    return x.cpu().numpy()


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def test_indexer_kat_on_device(kat):
    k = kat["misc_indexer"]
    A = dev(np.array(k["A"]))
    for ix in (et.SparseIndexer(), et.DenseIndexer()):
        for _ in range(2):
            et.index_(ix, A, int(max(k["A"])))
            assert host(ix.cumulative).tolist() == k["expected_cumulative"]
            assert host(ix.map).tolist() == k["expected_map"]


@pytest.mark.parametrize("shape", [(1000,), (300, 20), (64, 1)])
def test_indexer_random_vs_oracle(oracle, shape):
    rng = np.random.default_rng(sum(shape))
    I = rng.integers(1, 200, shape)
    cum, mp = oracle.index_build(I, 199)
    ix = et.index_(et.Indexer(), dev(I), 199)
    assert bits_equal(host(ix.cumulative), cum)
    assert bits_equal(host(ix.map), mp)


def test_readme_update_kat(kat):
    k = kat["readme_update"]
    A = et.SimpleEmbedding(torch.zeros((4, 4), dtype=torch.float32, device=DEV))
    y, back = et.rrule(et.lookup, A, dev(np.array(k["indices"])))
    assert not host(y).any()
    delta = dev(np.asarray(k["delta_columns"], np.float32))
    g = back(delta)
    assert g[0] is et.NoTangent() and g[2] is et.NoTangent()
    assert isinstance(g[1], et.SparseEmbeddingUpdate)
    et.update_(et.Descent(k["eta"]), A, g[1])
    assert np.allclose(host(A.data), np.asarray(k["expected_columns_as_printed"], np.float32),
                       rtol=1e-6, atol=0)


@pytest.mark.parametrize("dim", [64, 80, 128, 256])
@pytest.mark.parametrize("static", [True, False])
@pytest.mark.parametrize("reducing", [False, True])
def test_update_exact_vs_oracle(oracle, dim, static, reducing):
    """Single-table Descent update: bit-identical to the oracle in both the fused
    (Static <= 512 B) and unfused (generic) forms; isapprox to the dense update."""
    rng = np.random.default_rng(dim * 2 + static)
    ncols = 100
    base = rng.standard_normal((ncols, dim)).astype(np.float32)
    I = rng.integers(1, ncols + 1, (ncols, 10) if reducing else (ncols,))
    delta = rng.standard_normal((ncols, dim)).astype(np.float32)
    A = et.SimpleEmbedding(dev(base), et.Static(dim) if static else et.Dynamic)
    from embtab.tables import fused_update_path

    g = et.SparseEmbeddingUpdate(A.lookup_type, dev(delta), dev(I))
    et.update_(et.Descent(10.0), A, g)
    ref = base.copy()
    oracle.sgd(ref, delta, I, 10.0, fused=fused_update_path(A))
    assert bits_equal(host(A.data), ref)
    # uncompress vs a dense scatter (test/update.jl:44-45)
    dense = host(et.uncompress(g, ncols))
    acc = np.zeros((ncols, dim), np.float64)
    Ib = I.reshape(ncols, -1)
    for j in range(ncols):
        for c in Ib[j]:
            acc[c - 1] += delta[j]
    assert np.allclose(dense, acc, rtol=3.45e-4, atol=1e-4)


def test_update_hot_rows_chunked_vs_exact(oracle):
    """Zipf-skewed indices.  Exact mode: bit-identical to the reference's serial sum
    (north_star's 1e-6-relative bound, met with zero error).  Split mode: columns with
    at most ET_SGD_CHUNK occurrences are bit-identical too; longer occurrence lists are
    summed as ordered partial sums (deterministic), whose error is bounded by 1e-6 of the
    summation-error scale |w| + eta * sum|delta| of the exact (fp64) update and is no
    larger — absolute or relative to the exact update — than the serial fp32 sum's own
    error: the chunked result is as close to the true update as the reference's."""
    rng = np.random.default_rng(12)
    ncols, dim, B, P = 5000, 128, 4096, 20
    base = rng.standard_normal((ncols, dim)).astype(np.float32)
    z = np.minimum(rng.zipf(1.05, (B, P)), ncols)
    perm = rng.permutation(ncols) + 1
    I = perm[z - 1]
    delta = rng.standard_normal((B, dim)).astype(np.float32)
    ref = base.copy()
    oracle.sgd(ref, delta, I, 0.1, fused=True)
    counts = np.bincount(I.ravel(), minlength=ncols + 1)
    assert counts.max() > 4 * CHUNK  # the test really has split rows
    res = {}
    for exact in (True, False):
        A = et.SimpleEmbedding(dev(base), et.Static(dim))
        et.update_(et.Descent(0.1), A, et.SparseEmbeddingUpdate(A.lookup_type, dev(delta),
                                                                dev(I)), exact=exact)
        res[exact] = host(A.data)
    assert bits_equal(res[True], ref)
    hot = counts[1:] > CHUNK
    assert bits_equal(res[False][~hot], ref[~hot])
    # Tolerance for the reassociated hot-column sums, measured against the EXACT (fp64)
    # update: 1e-6 relative to the magnitude of the computation's inputs,
    # |w| + eta * sum_k |delta_k| (the summation error-bound scale).  The reference's own
    # serial fp32 sum is only about that accurate on a 50k-occurrence column; the chunked
    # sum is measured at ~10x closer to exact there (scratch diagnostics).
    acc = np.zeros((ncols, dim), np.float64)
    np.add.at(acc, I.ravel() - 1, np.repeat(delta.astype(np.float64), P, axis=0))
    absacc = np.zeros((ncols, dim), np.float64)
    np.add.at(absacc, I.ravel() - 1, np.repeat(np.abs(delta).astype(np.float64), P, axis=0))
    eta = np.float64(np.float32(0.1))
    exact_upd = base.astype(np.float64) - eta * acc
    scale = np.abs(base.astype(np.float64)) + eta * absacc
    err_chunked = np.abs(res[False].astype(np.float64) - exact_upd)
    err_serial = np.abs(ref.astype(np.float64) - exact_upd)
    assert np.all(err_chunked <= 1e-6 * scale)
    assert err_chunked[hot].max() <= err_serial[hot].max()
    big = hot[:, None] & (np.abs(exact_upd) > 1.0)
    rel_chunked = (err_chunked / np.abs(exact_upd))[big]
    rel_serial = (err_serial / np.abs(exact_upd))[big]
    assert big.any() and rel_chunked.max() <= rel_serial.max()
    # deterministic: the chunked result repeats exactly
    A = et.SimpleEmbedding(dev(base), et.Static(dim))
    et.update_(et.Descent(0.1), A, et.SparseEmbeddingUpdate(A.lookup_type, dev(delta), dev(I)),
               exact=False)
    assert bits_equal(host(A.data), res[False])


def test_update_partitions_exact(oracle):
    """test/update.jl:90-120: 4 IndexerView splits give exactly the unsplit update."""
    rng = np.random.default_rng(11)
    base = rng.standard_normal((100, 16)).astype(np.float32)
    delta = rng.standard_normal((512, 16)).astype(np.float32)
    I = rng.integers(1, 101, 512)
    for ixcls in (et.SparseIndexer, et.DenseIndexer):
        A = et.SimpleEmbedding(dev(base), et.Static(16))
        g = et.SparseEmbeddingUpdate(A.lookup_type, dev(delta), dev(I))
        ix = et.index_(ixcls(), g.indices, 100)
        et.update_(A, g, ix, 1.0)
        Bt = et.SimpleEmbedding(dev(base), et.Static(16))
        for s in range(1, 5):
            et.update_(Bt, g, et.IndexerView(ix, 4, s), 1.0)
        assert bits_equal(host(A.data), host(Bt.data))
        ref = base.copy()
        oracle.sgd(ref, delta, I, 1.0, fused=True)
        assert bits_equal(host(A.data), ref)


@pytest.mark.parametrize("fused_dims", [(128, 128, 64), (16, 256, 80)])
def test_multi_table_update_vs_oracle(oracle, fused_dims):
    """Multi-table update! (src/sparseupdate.jl:199-238) through Preallocation grads
    (strided deltas, ld = k + sum D), Static and Dynamic tables mixed."""
    rng = np.random.default_rng(sum(fused_dims))
    k, B, P = 8, 256, 20
    rows = [300, 1000, 50]
    hs = [rng.standard_normal((r, d)).astype(np.float32) for r, d in zip(rows, fused_dims)]
    statics = [True, True, False]
    tabs = [et.SimpleEmbedding(dev(h), et.Static(h.shape[1]) if s else et.Dynamic)
            for h, s in zip(hs, statics)]
    hidx = [rng.integers(1, r + 1, (B, P)) for r in rows]
    y, back = et.rrule(et.maplookup, et.PreallocationStrategy(k), tabs, [dev(i) for i in hidx])
    delta = rng.standard_normal(tuple(y.shape)).astype(np.float32)
    grads = back(dev(delta))[2]
    et.update_(et.Descent(0.1), tabs, grads, [et.Indexer() for _ in tabs])
    from embtab.tables import fused_update_path

    refs = [h.copy() for h in hs]
    offs = np.cumsum([k] + list(fused_dims[:-1]))
    oracle.sgd_multi(refs, delta, hidx, 0.1, [fused_update_path(t) for t in tabs], num_splits=4,
                     nthreads=4, delta_offsets=offs)
    for t in range(3):
        assert bits_equal(host(tabs[t].data), refs[t]), f"table {t}"


def test_map_gradients_structure():
    """test/map.jl:109-177: grads through maplookup and PreallocationStrategy (with and
    without prepended rows) carry the forward indices and equal deltas."""
    rng = np.random.default_rng(0)
    dims = [(5, 5), (5, 10), (5, 15)]
    tabs = [et.SimpleEmbedding(dev(rng.random((c, d), dtype=np.float32))) for d, c in dims]
    I = [dev(rng.integers(1, c + 1, 5)) for _, c in dims]
    y, back = et.rrule(et.maplookup, et.DefaultStrategy(), tabs, I)
    deltas = [torch.randn_like(o) for o in y]
    g1 = back(deltas)[2]
    for k in (0, 20):
        yp, backp = et.rrule(et.maplookup, et.PreallocationStrategy(k), tabs, I)
        big = torch.zeros_like(yp)
        big[:, k:] = torch.cat(deltas, 1)
        g2 = backp(big)[2]
        for a, b, i in zip(g1, g2, I):
            assert isinstance(b, et.SparseEmbeddingUpdate)
            assert b.indices is i and a.indices is i
            assert torch.equal(a.delta, b.delta)


def test_update_oob_skipped():
    et.check_errors()
    A = et.SimpleEmbedding(torch.zeros((10, 16), dtype=torch.float32, device=DEV), et.Static(16))
    I = torch.tensor([1, 11, 2], dtype=torch.int64, device=DEV)
    d = torch.ones((3, 16), dtype=torch.float32, device=DEV)
    et.update_(et.Descent(1.0), A, et.SparseEmbeddingUpdate(A.lookup_type, d, I))
    assert et.check_errors() == 1
    out = host(A.data)
    assert (out[0] == -1).all() and (out[1] == -1).all() and not out[2:].any()


# --- Float64 / Float16 / BFloat16 tables ---------------------------------------------------
# No reference test covers them (parity unpinned by the reference); the oracle's typed
# model (oracle/embtab_oracle.c, "update of Float64 / Float16 / BFloat16 tables") is
# the definition, and the HIP path must match it bit for bit.

def _typed(rng, shape, kind):
    x = rng.standard_normal(shape).astype(np.float32)
    if kind == "bf16":
        from oracle import f32_to_bf16
        return f32_to_bf16(x)
    return x.astype({"f64": np.float64, "f16": np.float16, "f16acc": np.float16}[kind])


def _dev_typed(a, kind):
    t = dev(a)
    return t.view(torch.bfloat16) if kind == "bf16" else t


def _host_bits(t):
    return host(t.view(torch.int16)) if t.dtype in (torch.float16, torch.bfloat16) else host(t)


@pytest.mark.parametrize("kind", ["f64", "f16", "f16acc", "bf16"])
@pytest.mark.parametrize("dim,static", [(64, True), (128, True), (40, False)])
@pytest.mark.parametrize("exact", [True, False])
def test_update_typed_vs_oracle(oracle, kind, dim, static, exact):
    rng = np.random.default_rng(dim + len(kind))
    ncols, B, P = 300, 256, 8
    base = _typed(rng, (ncols, dim), kind)
    delta = _typed(rng, (B, dim), kind)
    I = rng.integers(1, ncols + 1, (B, P))
    I[:, 0] = 7  # one column with ~256 occurrences, another with 768 (partials)
    I[:, 1:4] = 11
    A = et.SimpleEmbedding(_dev_typed(base, kind), et.Static(dim) if static else et.Dynamic)
    from embtab.tables import fused_update_path

    g = et.SparseEmbeddingUpdate(A.lookup_type, _dev_typed(delta, kind), dev(I))
    et.update_(et.Descent(0.1), A, g, exact=exact, f16_fp32_acc=kind == "f16acc")
    ref = base.copy()
    oracle.sgd(ref, delta, I, 0.1, fused=fused_update_path(A), bf16=kind == "bf16",
               f16_fp32_acc=kind == "f16acc")
    got = _host_bits(A.data)
    # columns with more than ET_SGD_CHUNK occurrences (11: 768; 7: 256 + its random
    # ones) are summed as ordered partials unless exact
    hot = np.bincount(I.ravel(), minlength=ncols + 1)[1:] > CHUNK
    assert hot[10]
    if exact:
        assert bits_equal(got, ref.view(got.dtype))
    else:
        assert bits_equal(got[~hot], ref.view(got.dtype)[~hot])
        w = got[hot].view(ref.dtype)
        r = ref[hot]
        if kind == "bf16":
            from oracle import bf16_to_f32
            w, r = bf16_to_f32(w), bf16_to_f32(r)
        tol = {"f64": 1e-12, "f16": 0.5, "f16acc": 5e-3, "bf16": 3e-2}[kind]
        assert np.allclose(np.asarray(w, np.float64), np.asarray(r, np.float64), rtol=tol,
                           atol=tol)


@pytest.mark.parametrize("kind", ["f64", "f16", "bf16"])
def test_multi_table_typed_and_indexer_view(oracle, kind):
    """Multi-table update! of typed tables (the generic path sees Float64 eta) and the
    IndexerView update of a typed table."""
    rng = np.random.default_rng(3)
    B, P, k = 200, 10, 4
    dims, rows = (32, 128, 64), (100, 400, 50)
    hs = [_typed(rng, (r, d), kind) for r, d in zip(rows, dims)]
    tabs = [et.SimpleEmbedding(_dev_typed(h, kind), et.Static(d) if t != 2 else et.Dynamic)
            for t, (h, d) in enumerate(zip(hs, dims))]
    hidx = [rng.integers(1, r + 1, (B, P)) for r in rows]
    ld = k + sum(dims)
    big = _typed(rng, (B, ld), kind)
    offs = np.cumsum([k] + list(dims[:-1]))
    gbig = _dev_typed(big, kind)
    grads = [et.SparseEmbeddingUpdate(A.lookup_type, gbig[:, o:o + d], dev(i))
             for A, o, d, i in zip(tabs, offs, dims, hidx)]
    et.update_(et.Descent(0.25), tabs, grads, [et.Indexer() for _ in tabs])
    from embtab.tables import fused_update_path

    refs = [h.copy() for h in hs]
    oracle.sgd_multi(refs, big, hidx, 0.25, [fused_update_path(t) for t in tabs],
                     delta_offsets=offs, bf16=kind == "bf16")
    for t in range(3):
        assert bits_equal(_host_bits(tabs[t].data), refs[t].view(_host_bits(tabs[t].data).dtype))
    # IndexerView splits of a typed table == the single-table oracle update with alpha
    base = _typed(rng, (100, 48), kind)
    delta = _typed(rng, (300, 48), kind)
    I = rng.integers(1, 101, 300)
    A = et.SimpleEmbedding(_dev_typed(base, kind), et.Static(48))
    g = et.SparseEmbeddingUpdate(A.lookup_type, _dev_typed(delta, kind), dev(I))
    ix = et.index_(et.Indexer(), g.indices, 100)
    for s in range(1, 5):
        et.update_(A, g, et.IndexerView(ix, 4, s), 0.5)
    ref = base.copy()
    oracle.sgd(ref, delta, I, 0.5, fused=fused_update_path(A), bf16=kind == "bf16")
    assert bits_equal(_host_bits(A.data), ref.view(_host_bits(A.data).dtype))


def test_forward_and_update_capture_in_a_hip_graph(oracle):
    """Every launch of maplookup! and update! is stream-ordered with device-side counts
    (no host synchronisation, no allocation once the workspace exists), so a whole
    training step can be captured in a HIP graph and replayed: the replay gives the
    same bits as eager execution."""
    rng = np.random.default_rng(31)
    dims, rows, B, P = (64, 128, 128), (500, 3000, 40), 512, 12
    hs = [rng.standard_normal((r, d)).astype(np.float32) for r, d in zip(rows, dims)]
    idx = [dev(rng.integers(1, r + 1, (B, P))) for r in rows]
    delta = dev(rng.standard_normal((B, sum(dims))).astype(np.float32))

    def step(tabs, dst):
        et.maplookup_(et.PreallocationStrategy(0), dst, tabs, idx)
        offs = np.cumsum([0] + list(dims[:-1]))
        grads = [et.SparseEmbeddingUpdate(t.lookup_type, delta[:, o:o + d], i)
                 for t, o, d, i in zip(tabs, offs, dims, idx)]
        et.update_(et.Descent(0.05), tabs, grads, [et.Indexer() for _ in tabs])

    eager = [et.SimpleEmbedding(dev(h), et.Static(h.shape[1])) for h in hs]
    out_e = torch.empty((B, sum(dims)), dtype=torch.float32, device=DEV)
    step(eager, out_e)
    step(eager, out_e)

    graphed = [et.SimpleEmbedding(dev(h), et.Static(h.shape[1])) for h in hs]
    out_g = torch.empty_like(out_e)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up outside the capture (workspace allocation)
        scratch = [et.SimpleEmbedding(dev(h), et.Static(h.shape[1])) for h in hs]
        step(scratch, torch.empty_like(out_e))
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step(graphed, out_g)
    g.replay()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out_g, out_e)
    for a, b in zip(graphed, eager):
        assert torch.equal(a.data, b.data)


@pytest.mark.parametrize("dim", [20, 40, 96, 200, 1504])
def test_update_masked_vector_dims(oracle, dim):
    """Float32 tables of any dim that is a multiple of 4 run the vector SGD kernels at
    the next power-of-two capacity (masked): exact mode bit-identical to the oracle,
    chunked mode bit-identical on every column with <= ET_SGD_CHUNK occurrences."""
    rng = np.random.default_rng(dim)
    ncols, B, P = 400, 300, 6
    base = rng.standard_normal((ncols, dim)).astype(np.float32)
    delta = rng.standard_normal((B, dim)).astype(np.float32)
    I = rng.integers(1, ncols + 1, (B, P))
    I[:, :3] = 9  # column 9: 900 occurrences -> chunked partial sums unless exact
    ref = base.copy()
    oracle.sgd(ref, delta, I, 0.3, fused=dim * 4 <= 512)
    for exact in (True, False):
        A = et.SimpleEmbedding(dev(base), et.Static(dim))
        et.update_(et.Descent(0.3), A, et.SparseEmbeddingUpdate(A.lookup_type, dev(delta),
                                                                dev(I)), exact=exact)
        got = host(A.data)
        if exact:
            assert bits_equal(got, ref)
        else:
            keep = np.ones(ncols, bool)
            keep[8] = False
            assert bits_equal(got[keep], ref[keep])
            # the chunked column against the exact fp64 update, at the summation
            # error-bound scale 1e-6 * (|w| + eta * sum |delta|) (as in the hot-row test)
            occ = (I == 9).sum(1)
            exact64 = base[8].astype(np.float64) - np.float64(np.float32(0.3)) * (
                occ[:, None] * delta.astype(np.float64)).sum(0)
            scale = np.abs(base[8]) + 0.3 * (occ[:, None] * np.abs(delta)).sum(0)
            assert np.all(np.abs(got[8] - exact64) <= 1e-6 * scale)


@pytest.mark.parametrize("dim", [16, 32, 64, 128, 256, 512])
def test_update_repeated_rows_in_bags(oracle, dim):
    """Tiny tables: every bag repeats its rows many times, so every column's occurrence
    list is long runs of equal bags (one delta load per run, added `run` times); exact mode
    bit-identical to the oracle, sorted and unsorted bags.  Tables of 3 and 7 rows with pools
    of 40 and 70 are early-chain tables (at most 128 rows, pool at most 255), so it is the
    early-chain planner (k_ec_count / k_ec_plan / k_ec_emit) that cuts these runs from
    per-bag byte counts; the regular plan's handling of long runs in the sorted list is pinned
    by tests/test_gpu_sgd_thresholds.py."""
    rng = np.random.default_rng(100 + dim)
    for ncols, B, P in ((3, 257, 40), (7, 130, 70)):
        base = rng.standard_normal((ncols, dim)).astype(np.float32)
        delta = rng.standard_normal((B, dim)).astype(np.float32)
        I = np.sort(rng.integers(1, ncols + 1, (B, P)), axis=1)
        I[::3] = rng.integers(1, ncols + 1, (I[::3].shape))  # unsorted bags as well
        ref = base.copy()
        oracle.sgd(ref, delta, I, 0.25, fused=dim * 4 <= 512)
        A = et.SimpleEmbedding(dev(base), et.Static(dim))
        et.update_(et.Descent(0.25), A, et.SparseEmbeddingUpdate(A.lookup_type, dev(delta),
                                                                 dev(I)), exact=True)
        assert bits_equal(host(A.data), ref)


@pytest.mark.parametrize("exact,hot", [(False, False), (False, True), (True, False)])
def test_phased_update_index_overlapping_forward(oracle, exact, hot):
    """PhasedUpdate: the index phase (src/sparseupdate.jl:210-213) runs on a side stream
    while maplookup! runs on the main stream, the update phase (:216-237) after both.
    Bit-identical to the one-call update_ (hot rows split into chunks, a Dynamic table
    on the generic path, a Float64 group), the index arrays may be overwritten once the
    index phase is done, and a second update_ reuses the same index work."""
    rng = np.random.default_rng(77 + exact + 2 * hot)
    dims, rows, B, P = (128, 64, 40), (2000, 7, 300), 1024, 20
    hs = [rng.standard_normal((r, d)).astype(np.float32) for r, d in zip(rows, dims)]
    statics = [True, True, False]
    hidx = [rng.integers(1, r + 1, (B, P)) for r in rows]
    hidx[0][:, :3] = 5  # a hot column: 3072 occurrences, several chunks
    delta = dev(rng.standard_normal((B, sum(dims))).astype(np.float32))
    offs = np.cumsum([0] + list(dims[:-1]))
    h64 = rng.standard_normal((500, 32))
    i64 = rng.integers(1, 501, (B, 8))
    d64 = dev(rng.standard_normal((B, 32)))

    def make():
        tabs = [et.SimpleEmbedding(dev(h), et.Static(h.shape[1]) if s else et.Dynamic)
                for h, s in zip(hs, statics)]
        tabs.append(et.SimpleEmbedding(dev(h64), et.Static(32)))
        idx = [dev(i) for i in hidx] + [dev(i64)]
        grads = [et.SparseEmbeddingUpdate(t.lookup_type, delta[:, o:o + d], i)
                 for t, o, d, i in zip(tabs, offs, dims, idx)]
        grads.append(et.SparseEmbeddingUpdate(tabs[3].lookup_type, d64, idx[3]))
        return tabs, idx, grads

    opt = et.Descent(0.05)
    ref_tabs, _, ref_grads = make()
    et.update_(opt, ref_tabs, ref_grads, None, exact=exact, hot_pass=hot)
    et.update_(opt, ref_tabs, ref_grads, None, exact=exact, hot_pass=hot)

    tabs, idx, grads = make()
    pu = et.PhasedUpdate(tabs, grads, exact=exact, hot_pass=hot)
    out = torch.empty((B, sum(dims)), dtype=torch.float32, device=DEV)
    main = torch.cuda.current_stream()
    side = torch.cuda.Stream()
    side.wait_stream(main)
    pu.index_(side)
    et.maplookup_(et.PreallocationStrategy(0), out, tabs[:3], idx[:3])  # concurrent
    main.wait_stream(side)
    for i in idx:
        i.fill_(1)  # phase 2 never reads the indices again
    pu.update_(opt)
    pu.update_(opt)
    torch.cuda.synchronize()
    for t, (a, b) in enumerate(zip(tabs, ref_tabs)):
        assert torch.equal(a.data, b.data), f"table {t}"
    if exact:
        from embtab.tables import fused_update_path

        refs = [h.copy() for h in hs]
        hd = host(delta)
        for _ in range(2):
            oracle.sgd_multi(refs, hd, hidx, 0.05, [fused_update_path(t) for t in tabs[:3]],
                             num_splits=4, nthreads=4, delta_offsets=offs)
        for t in range(3):
            assert bits_equal(host(tabs[t].data), refs[t]), f"table {t} vs oracle"


def test_phased_update_requires_index_phase():
    tab = et.SimpleEmbedding(dev(np.ones((10, 16), np.float32)), et.Static(16))
    g = et.SparseEmbeddingUpdate(tab.lookup_type, torch.ones((4, 16), device=DEV),
                                 dev(np.ones((4, 2), np.int64)))
    with pytest.raises(et.ArgumentError):
        et.PhasedUpdate([tab], [g]).update_(et.Descent(0.1))


def _fp64_update_and_scale(base, delta, I, eta32=0.1):
    """The exact (fp64) Descent update of one table and its error-bound scale
    |w| + eta * sum |delta| (see test_update_hot_rows_chunked_vs_exact)."""
    ncols = base.shape[0]
    ok = (I >= 1) & (I <= ncols)
    bags = np.repeat(np.arange(I.shape[0]), I.shape[1]).reshape(I.shape)
    acc = np.zeros(base.shape, np.float64)
    np.add.at(acc, I[ok] - 1, delta.astype(np.float64)[bags[ok]])
    absacc = np.zeros(base.shape, np.float64)
    np.add.at(absacc, I[ok] - 1, np.abs(delta).astype(np.float64)[bags[ok]])
    eta = np.float64(np.float32(eta32))
    return base.astype(np.float64) - eta * acc, np.abs(base.astype(np.float64)) + eta * absacc


def test_update_hot_column_pass_multi_table(oracle):
    """The bag-major hot-column pass (opt-in ET_FLAG_SGD_HOT_PASS) (k_hot_pick / k_sgd_hot / k_hot_combine): several
    dim-128 tables through a Preallocation-strided gradient, a paged table, a batch that
    is not a multiple of the 1024-bag window or the 32-bag batch, pool 13 (not a multiple
    of 4), out-of-range indices, and a table with more multi-chunk columns than hot slots
    (only the columns above the length threshold go bag-major).  Columns outside the hot
    set are bit-identical to the reference's serial sum, hot ones within the summation
    bound, and the result repeats bit for bit."""
    rng = np.random.default_rng(2024)
    B, P, D = 5000, 13, 128
    rows = [3000, 170, 40000]
    bases = [rng.standard_normal((r, D)).astype(np.float32) for r in rows]
    I0 = np.minimum(rng.zipf(1.1, (B, P)), rows[0])
    I0 = (rng.permutation(rows[0]) + 1)[I0 - 1]
    I1 = rng.integers(1, 151, (B, P))  # 150 columns of ~430 occurrences ...
    I1[:, :2] = rng.integers(151, 154, (B, 2))  # ... and 3 of ~3300
    I1[rng.random((B, P)) < 0.3] = rng.integers(151, 171, 1)[0]  # one column of ~19500
    I2 = np.minimum(rng.zipf(1.3, (B, P)), rows[2])
    I2[7, 3], I2[99, 0], I2[4999, 12] = 0, rows[2] + 1, -5  # skipped
    hidx = [I0, I1, I2]
    ld = 8 + 3 * D
    delta = rng.standard_normal((B, ld)).astype(np.float32)

    def run():
        tabs = [et.SimpleEmbedding(dev(bases[0]), et.Static(D)),
                et.SplitEmbedding(dev(bases[1]), 64),
                et.SimpleEmbedding(dev(bases[2]), et.Static(D))]
        dd = dev(delta)
        grads = [et.SparseEmbeddingUpdate(t.lookup_type, dd[:, 8 + k * D:8 + (k + 1) * D],
                                          dev(i)) for k, (t, i) in enumerate(zip(tabs, hidx))]
        # exact=False: the exact mode (the default since ABI v9) has no hot-column pass
        et.update_(et.Descent(0.1), tabs, grads, None, exact=False, hot_pass=True)
        return [host(t.to_dense() if isinstance(t, et.SplitEmbedding) else t.data)
                for t in tabs]

    out = run()
    assert all(bits_equal(a, b) for a, b in zip(out, run()))
    # the oracle gets the skipped entries redirected to an unused column, left out below
    spare = int(np.flatnonzero(np.bincount(np.clip(I2, 0, rows[2]).ravel(),
                                           minlength=rows[2] + 1)[1:] == 0)[0]) + 1
    oidx = [I0, I1, np.where((I2 >= 1) & (I2 <= rows[2]), I2, spare)]
    assert bits_equal(out[2][spare - 1], bases[2][spare - 1])
    for k in range(3):
        ref = bases[k].copy()
        oracle.sgd(ref, np.ascontiguousarray(delta[:, 8 + k * D:8 + (k + 1) * D]), oidx[k],
                   0.1, fused=True)
        counts = np.bincount(oidx[k].ravel(), minlength=rows[k] + 1)
        short = counts[1:] <= CHUNK
        if k == 2:
            short[spare - 1] = False
        assert bits_equal(out[k][short], ref[short]), f"table {k}: short columns"
        exact_upd, scale = _fp64_update_and_scale(bases[k], delta[:, 8 + k * D:8 + (k + 1) * D],
                                                  hidx[k])
        assert np.all(np.abs(out[k].astype(np.float64) - exact_upd) <= 1e-6 * scale), k
    assert et.check_errors() == 6  # the 3 skipped entries, counted by both runs


def test_multi_table_update_phases_telemetry_and_indexers(oracle):
    """src/sparseupdate.jl:208-214: the multi-table update! indexes every table, calls
    telemetry_cb() between its index phase and its update phase, and leaves table i's
    Indexer in indexers[i].  Here: when the callback runs no table has been updated yet
    (the update phase is not enqueued), afterwards all are, and every indexers[i] equals
    et_index_build's Indexer of grads[i].indices (the reference's cumulative / map)."""
    rng = np.random.default_rng(208)
    dims, rows, B, P = [128, 64, 32], [500, 40, 3000], 300, 7
    hs = [rng.standard_normal((r, d)).astype(np.float32) for r, d in zip(rows, dims)]
    tabs = [et.SimpleEmbedding(dev(h), et.Static(h.shape[1])) for h in hs]
    hidx = [rng.integers(1, r + 1, (B, P)) for r in rows]
    delta = rng.standard_normal((B, sum(dims))).astype(np.float32)
    dd = dev(delta)
    offs = np.cumsum([0] + dims[:-1])
    grads = [et.SparseEmbeddingUpdate(t.lookup_type, dd[:, o:o + d], dev(i))
             for t, o, d, i in zip(tabs, offs, dims, hidx)]
    seen = []

    def telemetry():
        torch.cuda.synchronize()  # everything enqueued so far (the index phase) is done
        seen.append([bits_equal(host(t.data), h) for t, h in zip(tabs, hs)])

    indexers = [et.Indexer(), et.DenseIndexer(), et.SparseIndexer()]
    et.update_(et.Descent(0.1), tabs, grads, indexers, telemetry_cb=telemetry)
    assert seen == [[True, True, True]]
    for t in range(3):
        ref = hs[t].copy()
        oracle.sgd(ref, np.ascontiguousarray(delta[:, offs[t]:offs[t] + dims[t]]), hidx[t], 0.1,
                   fused=True)
        assert bits_equal(host(tabs[t].data), ref)
        fresh = et.index_(et.Indexer(), grads[t].indices, rows[t])
        assert torch.equal(indexers[t].cumulative, fresh.cumulative)
        assert torch.equal(indexers[t].map, fresh.map)
        assert indexers[t].nunique == fresh.nunique
        cum, mp = oracle.index_build(hidx[t], rows[t])
        assert np.array_equal(host(indexers[t].cumulative), cum)
        assert np.array_equal(host(indexers[t].map), mp)


def test_indexers_snapshot_the_indices_of_their_update(oracle):
    """indexers[i] is table i's Indexer of the indices THAT update used
    (src/sparseupdate.jl:211-213), even when the caller refills the index buffer in
    place (the PreallocationPlan serving pattern) before reading it."""
    rng = np.random.default_rng(211)
    rows, B, P = [300, 77], 200, 9
    hs = [rng.standard_normal((r, 64)).astype(np.float32) for r in rows]
    tabs = [et.SimpleEmbedding(dev(h), et.Static(64)) for h in hs]
    hidx = [rng.integers(1, r + 1, (B, P)) for r in rows]
    idx = [dev(i) for i in hidx]
    dd = dev(rng.standard_normal((B, 128)).astype(np.float32))
    grads = [et.SparseEmbeddingUpdate(t.lookup_type, dd[:, 64 * k:64 * (k + 1)], i)
             for k, (t, i) in enumerate(zip(tabs, idx))]
    indexers = [et.Indexer(), et.Indexer()]
    et.update_(et.Descent(0.1), tabs, grads, indexers)
    for i, r in zip(idx, rows):  # refill in place before anyone reads the indexers
        i.copy_(torch.from_numpy(rng.integers(1, r + 1, (B, P))))
    for t in range(2):
        cum, mp = oracle.index_build(hidx[t], rows[t])
        assert np.array_equal(host(indexers[t].cumulative), cum)
        assert np.array_equal(host(indexers[t].map), mp)


def test_single_table_update_fills_its_indexer(oracle):
    """The single-table update!(opt, table, grad, indexer) indexes into `indexer` first
    (src/sparseupdate.jl:159-178: index!(indexer, update.indices, size(table, 2))), so a
    caller-supplied Indexer holds the reference's cumulative / map of THOSE indices after the
    call — from the update's own snapshot, even if the index buffer is refilled before it is
    read — and the table gets the oracle's update; Flux.Optimise.update! the same.  Vector
    and matrix indices, a hot column (a chain in the default exact mode)."""
    rng = np.random.default_rng(177)
    for shape in ((512, 20), (3000,)):
        R, D = 400, 64
        h = rng.standard_normal((R, D)).astype(np.float32)
        I = rng.integers(1, R + 1, shape)
        if len(shape) == 2:
            I[:, :3] = 7  # 1,536 occurrences of column 7
        delta = rng.standard_normal((shape[0], D)).astype(np.float32)
        for upd in (lambda *a: et.update_(*a), lambda o, A, g, ix: et.optimise_update_(o, A, g, ix)):
            A = et.SimpleEmbedding(dev(h), et.Static(D))
            Idev = dev(I)
            ix = et.Indexer()
            upd(et.Descent(0.1), A, et.SparseEmbeddingUpdate(A.lookup_type, dev(delta), Idev), ix)
            Idev.copy_(torch.from_numpy(rng.integers(1, R + 1, shape)))  # refilled in place
            cum, mp = oracle.index_build(I, R)
            assert np.array_equal(host(ix.cumulative), cum)
            assert np.array_equal(host(ix.map), mp)
            w = h.copy()
            oracle.sgd(w, delta, I, 0.1, fused=True)
            assert bits_equal(host(A.data), w)


def test_hot_pass_with_unaligned_preallocation_gradient(oracle):
    """hot_pass=True on a Preallocation gradient whose row blocks are not 16-byte aligned
    (prependrows k = 1): the host drops the hot-column pass for that group instead of
    the update phase refusing the plan of the index phase; the result is the ordinary
    update's (exact mode: the oracle's, bit for bit)."""
    rng = np.random.default_rng(17)
    rows, B, P, k = [400, 3000], 256, 20, 1
    hs = [rng.standard_normal((r, 128)).astype(np.float32) for r in rows]
    hidx = [rng.integers(1, r + 1, (B, P)) for r in rows]
    hidx[0][:, :4] = 5  # a column of 1024 occurrences (a hot-pass candidate)
    delta = rng.standard_normal((B, k + 256)).astype(np.float32)
    dd = dev(delta)
    for exact in (False, True):
        tabs = [et.SimpleEmbedding(dev(h), et.Static(128)) for h in hs]
        grads = [et.SparseEmbeddingUpdate(t.lookup_type, dd[:, k + 128 * j:k + 128 * (j + 1)],
                                          dev(i)) for j, (t, i) in enumerate(zip(tabs, hidx))]
        et.update_(et.Descent(0.1), tabs, grads, [et.Indexer(), et.Indexer()], exact=exact,
                   hot_pass=True)
        ref = [et.SimpleEmbedding(dev(h), et.Static(128)) for h in hs]
        rgrads = [et.SparseEmbeddingUpdate(t.lookup_type, dd[:, k + 128 * j:k + 128 * (j + 1)],
                                           dev(i)) for j, (t, i) in enumerate(zip(ref, hidx))]
        et.update_(et.Descent(0.1), ref, rgrads, None, exact=exact)
        for a, b in zip(tabs, ref):
            assert torch.equal(a.data, b.data)
        if exact:
            for j in range(2):
                w = hs[j].copy()
                oracle.sgd(w, np.ascontiguousarray(delta[:, k + 128 * j:k + 128 * (j + 1)]),
                           hidx[j], 0.1, fused=True)
                assert bits_equal(host(tabs[j].data), w)


def test_phased_hot_pass_null_delta_index_phase():
    """ET_FLAG_SGD_INDEX_ONLY with delta = NULL and the hot-column pass on: the index
    phase picks the hot columns from the tables alone, the update phase with an aligned
    gradient then equals the one-call update bit for bit; an update phase whose gradient
    cannot take the vector path the index phase planned for is refused (ET_ERR_ARG)
    before any device work."""
    import ctypes

    from embtab import _lib

    L = _lib.load()
    rng = np.random.default_rng(31)
    B, P, D, R = 3000, 13, 128, 400
    base = rng.standard_normal((R, D)).astype(np.float32)
    I = np.minimum(rng.zipf(1.1, (B, P)), R)
    delta = rng.standard_normal((B, D + 1)).astype(np.float32)
    dI, dd = dev(I), dev(delta)
    flags = _lib.ET_FLAG_NONTEMPORAL | _lib.ET_FLAG_SGD_HOT_PASS

    def desc(tab, dptr, ld):
        return _lib.UpdateDesc(tab.data_ptr(), D, R, D, P, dptr, ld, dI.data_ptr(), P, B, 0)

    one = dev(base)
    arr = (_lib.UpdateDesc * 1)(desc(one, dd.data_ptr(), D + 1))
    # reference run: the same table through the one-call update with an aligned copy of Δ
    al = dev(np.ascontiguousarray(delta[:, :D]))
    arr[0] = desc(one, al.data_ptr(), D)
    nb = ctypes.c_int64()
    _lib.check(L.et_sgd_workspace_size(ctypes.addressof(arr), 1, ctypes.byref(nb)))
    ws = torch.empty(nb.value, dtype=torch.uint8, device=DEV)
    st = _lib.stream_handle()
    _lib.check(L.et_sparse_sgd(_lib.ET_F32, ctypes.addressof(arr), 1, 0.1, flags, ws.data_ptr(),
                               ws.numel(), st))
    two = dev(base)
    arr[0] = desc(two, 0, D)  # phase 1 never reads the gradient
    _lib.check(L.et_sparse_sgd(_lib.ET_F32, ctypes.addressof(arr), 1, 0.1,
                               flags | _lib.ET_FLAG_SGD_INDEX_ONLY, ws.data_ptr(), ws.numel(), st))
    arr[0] = desc(two, dd.data_ptr() + 4, D + 1)  # misaligned: no vector path
    rc = L.et_sparse_sgd(_lib.ET_F32, ctypes.addressof(arr), 1, 0.1,
                         flags | _lib.ET_FLAG_SGD_APPLY_ONLY, ws.data_ptr(), ws.numel(), st)
    assert rc == -1 and b"hot-column" in L.et_last_error()
    arr[0] = desc(two, al.data_ptr(), D)
    _lib.check(L.et_sparse_sgd(_lib.ET_F32, ctypes.addressof(arr), 1, 0.1,
                               flags | _lib.ET_FLAG_SGD_APPLY_ONLY, ws.data_ptr(), ws.numel(), st))
    torch.cuda.synchronize()
    assert torch.equal(one, two)
    assert not torch.equal(one, dev(base))


def test_update_index_layouts_and_skew(oracle):
    """The key build's 16-byte path and its fallbacks, and skewed sort tiles: index
    buffers that are contiguous with a tail (n % 4 != 0), a strided view (ld_idx >
    pool), 8-byte aligned (storage offset 1), tables whose occurrence offset in a
    multi-table call is not a multiple of 4, and a 3-row table hit 90% by one column
    (one LDS address per run in the radix histogram).  Exact mode: bit-identical to
    the oracle; default mode on the same inputs: bit-identical wherever a column has
    at most ET_SGD_CHUNK occurrences."""
    from embtab.tables import fused_update_path

    rng = np.random.default_rng(77)

    def contiguous(B, P, R):
        return dev(rng.integers(1, R + 1, (B, P)))

    def strided(B, P, R):
        big = dev(rng.integers(1, R + 1, (B, P + 5)))
        return big[:, 2:2 + P]

    def offset1(B, P, R):
        buf = torch.empty(B * P + 1, dtype=torch.int64, device=DEV)
        v = buf[1:].view(B, P)
        v.copy_(dev(rng.integers(1, R + 1, (B, P))))
        assert v.data_ptr() % 16 == 8
        return v

    def skewed(B, P, R):
        I = np.where(rng.random((B, P)) < 0.9, 2, rng.integers(1, R + 1, (B, P)))
        return dev(I)

    cases = [(contiguous, 5, 3, 50), (strided, 7, 3, 40), (offset1, 33, 4, 60),
             (skewed, 1000, 20, 3), (contiguous, 129, 1, 500)]
    for exact in (True, False):
        # one table at a time
        for make, B, P, R in cases:
            base = rng.standard_normal((R, 128)).astype(np.float32)
            I = make(B, P, R)
            delta = rng.standard_normal((B, 128)).astype(np.float32)
            A = et.SimpleEmbedding(dev(base), et.Static(128))
            g = et.SparseEmbeddingUpdate(A.lookup_type, dev(delta), I)
            et.update_(et.Descent(0.5), A, g, exact=exact)
            ref = base.copy()
            Ih = host(I)
            oracle.sgd(ref, delta, Ih, 0.5, fused=fused_update_path(A))
            counts = np.bincount(Ih.reshape(-1), minlength=R + 1)[1:]
            ok = counts <= CHUNK if not exact else np.ones(R, bool)
            got = host(A.data)
            assert bits_equal(got[ok], ref[ok]), (make.__name__, B, P, R, exact)
            if not ok.all():  # chunked columns: both within 1e-6 of |w| + eta * sum|delta|
                absacc = np.zeros((R, 128))
                np.add.at(absacc, Ih.reshape(-1) - 1, np.repeat(np.abs(delta), P, axis=0))
                scale = np.abs(base) + 0.5 * absacc
                assert np.all(np.abs(got[~ok] - ref[~ok]) <= 2e-6 * scale[~ok])
        # all of them in one multi-table call (occurrence offsets 15, 36, 168, 20168)
        tabs, grads, refs, hs = [], [], [], []
        for make, B, P, R in [(c[0], 129, c[2], c[3]) for c in cases]:
            base = rng.standard_normal((R, 128)).astype(np.float32)
            I = make(B, P, R)
            delta = rng.standard_normal((B, 128)).astype(np.float32)
            A = et.SimpleEmbedding(dev(base), et.Static(128))
            tabs.append(A)
            grads.append(et.SparseEmbeddingUpdate(A.lookup_type, dev(delta), I))
            refs.append(base.copy())
            hs.append((host(I), delta))
        et.update_(et.Descent(0.5), tabs, grads, [et.Indexer() for _ in tabs], exact=exact)
        for A, ref, (Ih, delta) in zip(tabs, refs, hs):
            oracle.sgd(ref, delta, Ih, 0.5, fused=fused_update_path(A))
            counts = np.bincount(Ih.reshape(-1), minlength=ref.shape[0] + 1)[1:]
            ok = counts <= CHUNK if not exact else np.ones(ref.shape[0], bool)
            assert bits_equal(host(A.data)[ok], ref[ok])
    assert et.check_errors() == 0


@pytest.mark.parametrize("shift", [0, 4, 100])
def test_update_workspace_at_any_alignment(shift):
    """et_sparse_sgd lays its buffers out from the first 256-byte boundary of the
    caller's workspace (et_sgd_workspace_size includes the slack), so a workspace at a
    4-byte or 100-byte offset gives the same update as an aligned one."""
    import ctypes

    from embtab import _lib

    L = _lib.load()
    rng = np.random.default_rng(5)
    B, P, D, R = 2000, 20, 128, 700
    base = rng.standard_normal((R, D)).astype(np.float32)
    I = np.minimum(rng.zipf(1.2, (B, P)), R)
    delta = rng.standard_normal((B, D)).astype(np.float32)
    dI, dd = dev(I), dev(delta)
    outs = []
    for sh in (0, shift):
        tab = dev(base)
        arr = (_lib.UpdateDesc * 1)(_lib.UpdateDesc(tab.data_ptr(), D, R, D, P, dd.data_ptr(), D,
                                                    dI.data_ptr(), P, B, 0))
        nb = ctypes.c_int64()
        _lib.check(L.et_sgd_workspace_size(ctypes.addressof(arr), 1, ctypes.byref(nb)))
        ws = torch.empty(nb.value + sh, dtype=torch.uint8, device=DEV)
        _lib.check(L.et_sparse_sgd(_lib.ET_F32, ctypes.addressof(arr), 1, 0.1,
                                   _lib.ET_FLAG_NONTEMPORAL, ws.data_ptr() + sh, nb.value,
                                   _lib.stream_handle()))
        torch.cuda.synchronize()
        outs.append(tab)
    assert torch.equal(outs[0], outs[1])
    assert not torch.equal(outs[0], dev(base))


@pytest.mark.parametrize("kind", ["f32", "f64", "f16", "bf16"])
def test_default_mode_is_exact_for_every_dtype(oracle, kind):
    """The default update (exact=None, ET_FLAG_EXACT_IF_FAST) is the exact mode for every
    dtype since ABI v9 (round 4: Float32 only, the split mode otherwise): the default's
    result equals exact=True and the oracle's serial update bit for bit."""
    rng = np.random.default_rng(11)
    ncols, B, P, dim = 64, 512, 8, 64
    to = (lambda a: a.astype(np.float32)) if kind == "f32" else (lambda a: a)
    base = to(_typed(rng, (ncols, dim), "f64" if kind == "f32" else kind))
    delta = to(_typed(rng, (B, dim), "f64" if kind == "f32" else kind))
    I = rng.integers(1, ncols + 1, (B, P))
    I[:, :3] = 5  # a column of 1536+ occurrences: split and exact differ
    dk = "f32" if kind == "f32" else kind
    res = {}
    for mode in (None, True, False):
        A = et.SimpleEmbedding(dev(base) if dk == "f32" else _dev_typed(base, dk), et.Static(dim))
        g = et.SparseEmbeddingUpdate(A.lookup_type,
                                     dev(delta) if dk == "f32" else _dev_typed(delta, dk), dev(I))
        et.update_(et.Descent(0.1), A, g, exact=mode)
        res[mode] = _host_bits(A.data)
    assert bits_equal(res[None], res[True])
    from embtab.tables import fused_update_path
    ref = base.copy()
    A = et.SimpleEmbedding(dev(base) if dk == "f32" else _dev_typed(base, dk), et.Static(dim))
    oracle.sgd(ref, delta, I, 0.1, fused=fused_update_path(A), bf16=kind == "bf16")
    assert bits_equal(res[None], ref.view(res[None].dtype))
