"""Weighted and mean-pooled bags on the GPU: the forward, the weight gradient and the weighted
sparse SGD against tests/weighted_ref.py (a literal numpy restatement of include/embtab.h)
and, where the contract reduces to it, against the existing oracle.  Comparisons are
``tobytes()`` equality unless said otherwise (the weight gradient has a derived bound)."""
import numpy as np
import pytest
import torch

import embtab as et
import weighted_ref as wr
from embtab.tables import Dynamic, Static, fused_update_path
from weighted_ref import ROWS, colptr_of, mix_lengths

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def dev(x, bf16=False):
    t = torch.from_numpy(np.ascontiguousarray(x).view(np.int16) if bf16
                         else np.ascontiguousarray(x)).to(DEV)
    return t.view(torch.bfloat16) if bf16 else t


def host(x):
    if x.dtype in (torch.bfloat16, torch.float16):
        return x.view(torch.int16).cpu().numpy().view(np.uint16 if x.dtype == torch.bfloat16
                                                      else np.float16)
    return x.cpu().numpy()


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def ragged(values, colptr):
    return et.RaggedIndices(dev(values), dev(colptr))


@pytest.fixture(scope="module")
def mix301():
    rng = np.random.default_rng(301)
    L = mix_lengths(301, rng)
    values = rng.integers(1, ROWS + 1, int(L.sum())).astype(np.int64)
    return L, values, rng.standard_normal(len(values)).astype(np.float32)


# --- 1. forward geometry ---------------------------------------------------------------------

@pytest.mark.parametrize("dim", [16, 128, 512, 1504, 20, 7])
def test_forward_geometry(mix301, dim):
    L, values, w = mix301
    table = np.random.default_rng(dim).standard_normal((ROWS, dim)).astype(np.float32)
    A = et.SimpleEmbedding(dev(table))
    W = et.WeightedIndices(ragged(values, colptr_of(L)), dev(w))
    want, _ = wr.forward(table, values, colptr_of(L), w)
    assert same(host(et.lookup(A, W)), want)
    assert et.destination(A, W).shape == (301, dim)
    assert same(host(et.lookup_(et.destination(A, W), A, W, nontemporal=False)), want)
    # a strided destination: columns 4 .. 4+D of a wider tensor, surroundings untouched
    wide = torch.full((301, dim + 9), -3.0, device=DEV)
    et.lookup_(wide[:, 4:4 + dim], A, W)
    g = host(wide)
    assert same(g[:, 4:4 + dim], want)
    assert (g[:, :4] == -3).all() and (g[:, 4 + dim:] == -3).all()
    # every bag empty (no entry at all, then unused capacity)
    for cap in (0, 5):
        E = et.WeightedIndices(ragged(values[:cap], np.ones(302, np.int64)), dev(w[:cap]))
        assert same(host(et.lookup(A, E)), np.zeros((301, dim), np.float32))
    assert et.check_errors() == 0


# --- 2. weights of 1.0 (and no weights) are the unweighted lookup, bit for bit ---------------

@pytest.mark.parametrize("kind", ["f32", "f16"])
@pytest.mark.parametrize("dim", [128, 24, 7])
def test_unit_weights_equal_the_ragged_lookup(mix301, kind, dim):
    L, values, _ = mix301
    table, _ = wr.typed(np.random.default_rng(2).standard_normal((ROWS, dim)), kind)
    A = et.SimpleEmbedding(dev(table))
    R = ragged(values, colptr_of(L))
    plain = torch.empty((301, dim), dtype=A.dtype, device=DEV)
    et.maplookup_(et.PreallocationStrategy(0), plain, [A], [R], f16_fp32_acc=kind == "f16")
    ones = torch.ones(len(values), device=DEV)
    assert same(host(et.lookup(A, et.WeightedIndices(R, ones))), host(plain))
    assert same(host(et.lookup(A, et.WeightedIndices(R))), host(plain))
    if kind == "f32":
        assert same(host(et.lookup(A, R)), host(plain))
    assert et.check_errors() == 0


# --- 3. signed zeros; an out-of-range first entry with a negative weight ----------------------

@pytest.mark.parametrize("dim", [16, 7])
def test_signed_zeros_and_out_of_range(dim):
    table = np.random.default_rng(3).standard_normal((ROWS, dim)).astype(np.float32)
    table[[4, 9]] = -0.0
    #        [1*-0]  [-1*oor, 2*x]  []  [-3*-0]  [-1*oor]  [1*-0, 1*-0]
    L = np.array([1, 2, 0, 1, 1, 2])
    values = np.array([5, ROWS + 1, 3, 10, 0, 5, 10], np.int64)
    w = np.array([1, -1, 2, -3, -1, 1, 1], np.float32)
    et.check_errors()
    got = host(et.lookup(et.SimpleEmbedding(dev(table)),
                         et.WeightedIndices(ragged(values, colptr_of(L)), dev(w))))
    want, ev = wr.forward(table, values, colptr_of(L), w)
    assert ev == 2 and et.check_errors() == 2
    assert same(got, want)
    s = np.signbit(got)
    assert s[0].all() and not s[2].any() and not s[3].any() and s[4].all() and s[5].all()
    assert same(got[1], (np.float32(2) * table[2]))


# --- 4. element types ------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["f64", "f16", "bf16"])
@pytest.mark.parametrize("dim", [64, 10])
def test_forward_element_types(kind, dim):
    rng = np.random.default_rng(4)
    B = 130
    L = mix_lengths(B, rng)
    values = rng.integers(1, ROWS + 1, int(L.sum())).astype(np.int64)
    table, bf16 = wr.typed(rng.standard_normal((ROWS, dim)), kind)
    w = rng.standard_normal(len(values)).astype(wr.acc_type(table, bf16))
    A = et.SimpleEmbedding(dev(table, bf16))
    R = ragged(values, colptr_of(L))
    want, _ = wr.forward(table, values, colptr_of(L), w, bf16=bf16)
    assert same(host(et.lookup(A, et.WeightedIndices(R, dev(w)))), want)
    # one-entry bags: T(w * x) carries two roundings (Float32, then the 16-bit type)
    one = np.nonzero(L == 1)[0]
    assert len(one) and same(host(et.lookup(A, et.WeightedIndices(R, dev(w))))[one], want[one])
    wantm, _ = wr.forward(table, values, colptr_of(L), mode="mean", bf16=bf16)
    assert same(host(et.lookup(A, et.WeightedIndices(R, mode="mean"))), wantm)
    # the weights' type is checked at the call
    other = torch.ones(len(values), device=DEV,
                       dtype=torch.float32 if kind == "f64" else torch.float64)
    with pytest.raises(et.ArgumentError):
        et.lookup(A, et.WeightedIndices(R, other))
    assert et.check_errors() == 0


def test_integer_and_quantised_tables_are_refused():
    I = dev(np.ones((4, 3), np.int64))
    W, M = et.WeightedIndices(I, torch.ones(4, 3, device=DEV)), et.WeightedIndices(I, mode="mean")
    for dt in (torch.int32, torch.int64):
        A = et.SimpleEmbedding(torch.ones((8, 16), dtype=dt, device=DEV))
        for X in (W, M):
            with pytest.raises(et.ArgumentError):
                et.lookup(A, X)
    Q = et.QuantizedEmbedding(torch.zeros((8, 20), dtype=torch.uint8, device=DEV), 16, 8)
    for X in (W, M):
        with pytest.raises(et.ArgumentError):
            et.lookup(Q, X)
    with pytest.raises(et.ArgumentError):
        et.maplookup(et.PreallocationStrategy(0), [Q], [W])


# --- 5. mean mode ------------------------------------------------------------------------------

@pytest.mark.parametrize("dim", [16, 128, 7])
def test_mean_mode(mix301, dim):
    L, values, _ = mix301
    assert (L == 3).any()  # 1/3 is not exact
    table = np.random.default_rng(5).standard_normal((ROWS, dim)).astype(np.float32)
    vals = values.copy()
    vals[int(colptr_of(L)[np.nonzero(L == 3)[0][0]]) - 1] = ROWS + 7  # counts in the length
    A = et.SimpleEmbedding(dev(table))
    et.check_errors()
    got = host(et.lookup(A, et.WeightedIndices(ragged(vals, colptr_of(L)), mode="mean")))
    want, ev = wr.forward(table, vals, colptr_of(L), mode="mean")
    assert ev == 1 and et.check_errors() == 1
    assert same(got, want)
    assert not np.signbit(got[0]).any() and not got[0].any()  # an empty bag writes +0


# --- 6. a fixed-pool (B, P) index is the ragged index it is --------------------------------------

@pytest.mark.parametrize("P", [1, 8, 20])
def test_fixed_pool_equals_ragged(P):
    rng = np.random.default_rng(6)
    B, dim = 301, 128
    table = rng.standard_normal((ROWS, dim)).astype(np.float32)
    I = rng.integers(1, ROWS + 1, (B, P)).astype(np.int64)
    w = rng.standard_normal((B, P)).astype(np.float32)
    A = et.SimpleEmbedding(dev(table))
    R = ragged(I.reshape(-1), 1 + P * np.arange(B + 1, dtype=np.int64))
    for flat in (False, True):
        got = host(et.lookup(A, et.WeightedIndices(dev(I), dev(w.reshape(-1) if flat else w))))
        assert same(got, host(et.lookup(A, et.WeightedIndices(R, dev(w.reshape(-1))))))
    want, _ = wr.forward(table, I.reshape(-1), 1 + P * np.arange(B + 1), w.reshape(-1))
    assert same(got, want)
    gm = host(et.lookup(A, et.WeightedIndices(dev(I), mode="mean")))
    assert same(gm, host(et.lookup(A, et.WeightedIndices(R, mode="mean"))))
    assert et.check_errors() == 0


# --- 7. storage: paged and column-pointer-only tables, forward and update ----------------------

@pytest.mark.parametrize("store", ["split64", "colptr_vec", "colptr_generic"])
def test_storage_forward_and_update(oracle, store):
    from test_gpu_ragged import ScatteredColumns

    rng = np.random.default_rng(7)
    B = 130
    D = 128 if store != "colptr_generic" else 10
    L = mix_lengths(B, rng)
    cp = colptr_of(L)
    values = rng.integers(1, ROWS + 1, int(L.sum())).astype(np.int64)
    w = rng.standard_normal(len(values)).astype(np.float32)
    table = rng.standard_normal((ROWS, D)).astype(np.float32)
    if store == "split64":
        A = et.SplitEmbedding(dev(table), 64)
        dense = lambda: host(A.to_dense())
    else:
        A = ScatteredColumns(table, D + (4 if store == "colptr_vec" else 3), rng)
        dense = A.dense
    W = et.WeightedIndices(ragged(values, cp), dev(w), weight_grad=True)
    y, back = et.rrule(et.lookup, A, W)
    assert same(host(y), wr.forward(table, values, cp, w)[0])
    delta = rng.standard_normal((B, D)).astype(np.float32)
    _, grad, dw = back(dev(delta))
    ref, mag = wr.weight_grad_f64(table, delta, values, cp)
    assert (np.abs(host(dw) - ref) <= wr.gamma(D + 1, 2.0 ** -24) * mag).all()
    et.update_(et.Descent(0.1), A, grad)
    E, cov = wr.expanded_gradient(delta, w, cp, len(values))
    oracle.sgd(table, E[cov], values[cov], 0.1, fused=fused_update_path(A))
    assert same(dense(), table)
    assert et.check_errors() == 0


# --- 8. a mixed Preallocation list -----------------------------------------------------------------

@pytest.mark.parametrize("k", [0, 16])
def test_mixed_preallocation_list(oracle, k):
    rng = np.random.default_rng(8)
    B, dims = 140, [16, 128, 128, 64, 20]
    tables = [rng.standard_normal((ROWS, d)).astype(np.float32) for d in dims]
    As = [et.SimpleEmbedding(dev(t)) for t in tables]
    La, Lb, Lc = (mix_lengths(B, rng) for _ in range(3))
    va, vb, vc = (rng.integers(1, ROWS + 1, int(x.sum())).astype(np.int64) for x in (La, Lb, Lc))
    Imat = rng.integers(1, ROWS + 1, (B, 12)).astype(np.int64)
    Ifix = rng.integers(1, ROWS + 1, (B, 5)).astype(np.int64)
    wb = rng.standard_normal(len(vb)).astype(np.float32)
    wf = rng.standard_normal((B, 5)).astype(np.float32)
    Ra = ragged(va, colptr_of(La))
    # plain matrix, RaggedIndices, weighted ragged, weighted fixed-pool, mean
    Is = [dev(Imat), Ra, et.WeightedIndices(ragged(vb, colptr_of(Lb)), dev(wb)),
          et.WeightedIndices(dev(Ifix), dev(wf)),
          et.WeightedIndices(ragged(vc, colptr_of(Lc)), mode="mean")]
    strat = et.PreallocationStrategy(k)
    dst = torch.full((B, k + sum(dims)), -3.0, device=DEV)
    et.maplookup_(strat, dst, As, Is)
    got = host(dst)
    offs = np.cumsum([k] + dims)
    assert (got[:, :k] == -3).all()  # the prepended rows are untouched
    # the unweighted blocks are bit-identical to a call without the weighted tables
    alone = torch.full((B, k + dims[0] + dims[1]), -3.0, device=DEV)
    et.maplookup_(strat, alone, As[:2], Is[:2])
    assert same(got[:, k:offs[2]], host(alone)[:, k:])
    want = [wr.forward(tables[2], vb, colptr_of(Lb), wb)[0],
            wr.forward(tables[3], Ifix.reshape(-1), 1 + 5 * np.arange(B + 1), wf.reshape(-1))[0],
            wr.forward(tables[4], vc, colptr_of(Lc), mode="mean")[0]]
    for t, wnt in zip((2, 3, 4), want):
        assert same(got[:, offs[t]:offs[t + 1]], wnt), t
    assert same(host(et.maplookup(strat, As, Is))[:, k:], got[:, k:])
    for y, t in zip(et.maplookup(et.DefaultStrategy(), As, Is), range(5)):
        assert same(host(y), got[:, offs[t]:offs[t + 1]])
    # only weighted tables; a plan called twice with the weights refilled in place
    plan = et.PreallocationPlan(strat, dst, As[2:], Is[2:])
    Is[2].weights.copy_(dev(2 * wb))
    out = host(plan())
    assert same(out[:, k:k + 128], wr.forward(tables[2], vb, colptr_of(Lb), 2 * wb)[0])
    assert et.check_errors() == 0


# --- 9. owned memory only ------------------------------------------------------------------------------

@pytest.mark.parametrize("dim", [128, 7])
def test_clamping_reads_and_writes_only_owned_memory(oracle, dim):
    from embtab.weighted import weight_grad

    rng = np.random.default_rng(9)
    B, CAP, PAD = 40, 500, 64
    table = rng.standard_normal((ROWS, dim)).astype(np.float32)
    delta = rng.standard_normal((B, dim)).astype(np.float32)
    # values, weights and dw are views inside larger buffers: a kernel that forgot to clamp
    # would read valid indices but NaN weights, and write over the sentinels
    vbuf = dev(rng.integers(1, ROWS + 1, PAD + CAP + PAD).astype(np.int64))
    wbuf = torch.full((PAD + CAP + PAD,), float("nan"), device=DEV)
    dwbuf = torch.full((PAD + CAP + PAD,), 7.5, device=DEV)
    vals, wts, dw = (x[PAD:PAD + CAP] for x in (vbuf, wbuf, dwbuf))
    L = rng.integers(5, 13, B)
    used = int(L.sum())
    assert used + 20 <= CAP
    w = np.full(CAP, np.nan, np.float32)         # the capacity tail of the weights holds NaN
    w[:used] = rng.standard_normal(used)
    wts.copy_(dev(w))
    values = host(vals)
    colptr = colptr_of(L)
    colptr[0] = -4                               # the first bag's lo needs clamping
    rg, clamps = wr.ranges(colptr, CAP)
    assert clamps == 1 and rg[0][0] == 0 and rg[-1][1] == used
    R = et.RaggedIndices(vals, dev(colptr))
    et.check_errors()
    A = et.SimpleEmbedding(dev(table))
    got = host(et.lookup(A, et.WeightedIndices(R, wts)))
    want, ev = wr.forward(table, values, colptr, w, nnz=CAP)
    assert ev == 1 and et.check_errors() == ev
    assert same(got, want) and np.isfinite(got).all()
    # a colptr that decreases inside and claims entries beyond the capacity (the forward
    # only: two bags then overlap, so a per-entry result has no single owner)
    bad = colptr_of(L)
    bad[-1] = 900
    bad[18] = bad[17] - 3
    wfin = np.where(np.isnan(w), np.float32(0.5), w)
    got = host(et.lookup(A, et.WeightedIndices(et.RaggedIndices(vals, dev(bad)), dev(wfin))))
    want, ev = wr.forward(table, values, bad, wfin, nnz=CAP)
    assert ev == 2 and et.check_errors() == ev and same(got, want)
    # weight gradient into the owned view: sentinels intact, the tail +0
    weight_grad(A, dev(delta), R, out=dw)
    assert et.check_errors() == 1
    h = host(dwbuf)
    assert (h[:PAD] == 7.5).all() and (h[PAD + CAP:] == 7.5).all()
    assert same(h[PAD + used:PAD + CAP], np.zeros(CAP - used, np.float32))  # +0, bit for bit
    ref, mag = wr.weight_grad_f64(table, delta, values, colptr, nnz=CAP)
    assert (np.abs(h[PAD:PAD + CAP] - ref) <= wr.gamma(dim + 1, 2.0 ** -24) * mag).all()
    # the update never reads the NaN tail either
    et.update_(et.Descent(0.1), A, et.SparseEmbeddingUpdate(A.lookup_type, dev(delta), R, wts))
    assert et.check_errors() == 1
    E, cov = wr.expanded_gradient(delta, w, colptr, CAP)
    assert cov.sum() == used
    ref_t = table.copy()
    oracle.sgd(ref_t, E[cov], values[cov], 0.1, fused=fused_update_path(A))
    assert same(host(A.data), ref_t) and np.isfinite(ref_t).all()
    assert same(host(wbuf), np.concatenate([np.full(PAD, np.nan, np.float32), w,
                                            np.full(PAD, np.nan, np.float32)]))


# --- 10. weight gradient ---------------------------------------------------------------------------

@pytest.mark.parametrize("dim,kind", [(16, "f32"), (128, "f32"), (1504, "f32"), (7, "f32"),
                                      (16, "f16"), (7, "f16"), (128, "bf16"), (7, "bf16"),
                                      (128, "f64"), (7, "f64")])
def test_weight_gradient_within_the_summation_bound(dim, kind):
    """|dw - ref| <= gamma_{D+1} * sum_f |delta_f * x_f| with ref in Float64 (longdouble for
    Float64 tables): holds for any order of summation, so it is derived, not tuned
    (tests/test_weighted_host.py checks three CPU orders on the same inputs)."""
    table, delta, values, colptr, bf16 = wr.wgrad_case(dim, kind)
    A = et.SimpleEmbedding(dev(table, bf16))
    R = ragged(np.concatenate([values, values[:9]]), colptr)  # a capacity tail of 9
    from embtab.weighted import weight_grad
    dw1 = host(weight_grad(A, dev(delta, bf16), R))
    dw2 = host(weight_grad(A, dev(delta, bf16), R))
    assert same(dw1, dw2)  # the same order from run to run
    assert dw1.dtype == (np.float64 if kind == "f64" else np.float32)
    assert same(dw1[len(values):], np.zeros(9, dw1.dtype))
    ref, mag = wr.weight_grad_f64(table, delta, values, colptr, bf16)
    u = 2.0 ** -53 if kind == "f64" else 2.0 ** -24
    bound = wr.gamma(dim + 1, u) * mag
    err = np.abs(dw1[:len(values)].astype(ref.dtype) - ref)
    print(f"dim {dim} {kind}: largest observed / bound on the GPU = {float((err / bound).max()):.4f}")
    assert (err <= bound).all()
    # an out-of-range index gives +0 and is counted
    bad = values.copy()
    bad[[0, 5]] = [0, ROWS + 1]
    et.check_errors()
    dwb = host(weight_grad(A, dev(delta, bf16), ragged(bad, colptr)))
    assert et.check_errors() == 2
    assert same(dwb[[0, 5]], np.zeros(2, dwb.dtype)) and same(dwb[6:], dw1[6:len(values)])


# --- 11. weighted SGD ----------------------------------------------------------------------------------

def hot_case(B, rng):
    """The length mix plus ten bags of 300 entries of one hot row (more than 256 entries in
    one serial column), a second row with 100 entries (more than 64), the other values from
    40 distinct rows."""
    L = mix_lengths(B, rng, extra=[300] * 10)
    cp = colptr_of(L)
    rows40 = rng.choice(ROWS, 40, replace=False) + 1
    values = rows40[rng.integers(2, 40, int(L.sum()))].astype(np.int64)
    hot = np.nonzero(L == 300)[0][1:]
    for j in hot:
        values[cp[j] - 1:cp[j + 1] - 1] = rows40[0]
    cold = np.nonzero(values != rows40[0])[0]
    values[rng.choice(cold, 100, replace=False)] = rows40[1]
    assert (values == rows40[0]).sum() >= 3000 and (values == rows40[1]).sum() == 100
    return L, values, rows40


@pytest.mark.parametrize("kind", ["f32", "f64"])
@pytest.mark.parametrize("dim,static", [(16, True), (16, False), (128, True), (128, False),
                                        (200, False), (1504, False)])
def test_weighted_sgd_equals_the_oracle_on_the_expanded_gradient(oracle, kind, dim, static):
    rng = np.random.default_rng(11 + dim)
    B = 257
    L, values, rows40 = hot_case(B, rng)
    cp = colptr_of(L)
    table, _ = wr.typed(rng.standard_normal((ROWS, dim)), kind)
    delta, _ = wr.typed(rng.standard_normal((B, dim)), kind)
    # a capacity tail: a row of its own (never written) and the hot row (adds nothing)
    lonely = int(np.setdiff1d(np.arange(1, ROWS + 1), values)[0])
    vals = np.concatenate([values, [lonely, rows40[0], lonely]]).astype(np.int64)
    w = rng.standard_normal(len(vals)).astype(table.dtype)
    w[len(values):] = np.nan
    lt = Static(dim) if static else Dynamic
    A = et.SimpleEmbedding(dev(table), lt)
    E, cov = wr.expanded_gradient(delta, w, cp, len(vals))
    assert cov.sum() == len(values)
    ref = table.copy()
    oracle.sgd(ref, E[cov], vals[cov], 0.1, fused=fused_update_path(A))
    g = et.SparseEmbeddingUpdate(lt, dev(delta), ragged(vals, cp), dev(w))
    et.update_(et.Descent(0.1), A, g)
    assert same(host(A.data), ref)
    assert same(ref[lonely - 1], table[lonely - 1])  # only in the tail: not written
    if kind == "f32":
        assert same(wr.sgd(table.copy(), delta, vals, cp, w, 0.1,
                           fused=fused_update_path(A))[rows40[:3] - 1], ref[rows40[:3] - 1])
    # the delta as a strided view, exact=True, temporal stores
    A = et.SimpleEmbedding(dev(table), lt)
    wide = torch.zeros((B, dim + 8), dtype=A.dtype, device=DEV)
    wide[:, 4:4 + dim] = dev(delta)
    et.update_(et.Descent(0.1), A, et.SparseEmbeddingUpdate(lt, wide[:, 4:4 + dim],
                                                           ragged(vals, cp), dev(w)),
               exact=True, nontemporal=False)
    assert same(host(A.data), ref)
    assert et.check_errors() == 0


@pytest.mark.parametrize("kind", ["f16", "bf16"])
@pytest.mark.parametrize("static", [True, False])
def test_weighted_sgd_16_bit_types(kind, static):
    rng = np.random.default_rng(12)
    B, D = 130, 64
    L, values, _ = hot_case(B, rng)
    cp = colptr_of(L)
    table, bf16 = wr.typed(rng.standard_normal((ROWS, D)), kind)
    delta, _ = wr.typed(0.05 * rng.standard_normal((B, D)), kind)
    w = rng.standard_normal(len(values)).astype(np.float32)
    lt = Static(D) if static else Dynamic
    A = et.SimpleEmbedding(dev(table, bf16), lt)
    g = et.SparseEmbeddingUpdate(lt, dev(delta, bf16), ragged(values, cp), dev(w))
    et.update_(et.Descent(0.1), A, g)
    ref = wr.sgd(table.copy(), delta, values, cp, w, 0.1, fused=fused_update_path(A), bf16=bf16)
    assert same(host(A.data), ref)
    assert not same(ref, table)
    assert et.check_errors() == 0


def test_update_multi_table_mixed(oracle):
    rng = np.random.default_rng(13)
    B, dims = 140, [16, 128, 64, 200]
    lts = [Static(16), Dynamic, Static(64), Dynamic]
    hs = [rng.standard_normal((ROWS, d)).astype(np.float32) for d in dims]
    As = [et.SimpleEmbedding(dev(h), lt) for h, lt in zip(hs, lts)]
    La, Lb = mix_lengths(B, rng), mix_lengths(B, rng)
    va = rng.integers(1, 60, int(La.sum())).astype(np.int64)
    vb = rng.integers(1, 60, int(Lb.sum())).astype(np.int64)
    Imat = rng.integers(1, 60, (B, 5)).astype(np.int64)
    Ifix = rng.integers(1, 60, (B, 3)).astype(np.int64)
    wb = rng.standard_normal(len(vb)).astype(np.float32)
    wf = rng.standard_normal((B, 3)).astype(np.float32)
    Ra = ragged(va, colptr_of(La))
    # ragged, plain matrix, weighted ragged (with dw), weighted fixed-pool
    Is = [Ra, dev(Imat), et.WeightedIndices(ragged(vb, colptr_of(Lb)), dev(wb), weight_grad=True),
          et.WeightedIndices(dev(Ifix), dev(wf))]
    strat = et.PreallocationStrategy(3)
    y, back = et.rrule(et.maplookup, strat, As, Is)
    delta = rng.standard_normal(tuple(y.shape)).astype(np.float32)
    _, _, grads, dIs = back(dev(delta))
    assert isinstance(dIs, list) and [isinstance(d, et.NoTangent) for d in dIs] == [
        True, True, False, True]
    assert grads[0].weights is None and grads[1].weights is None
    assert grads[2].weights is not None and grads[3].weights.shape == (B * 3,)
    offs = np.cumsum([3] + dims)
    blk = lambda t: np.ascontiguousarray(delta[:, offs[t]:offs[t + 1]])
    ref, mag = wr.weight_grad_f64(hs[2], blk(2), vb, colptr_of(Lb))
    assert dIs[2].shape == (len(vb),)
    assert (np.abs(host(dIs[2]) - ref) <= wr.gamma(64 + 1, 2.0 ** -24) * mag).all()
    indexers = [et.Indexer() for _ in As]
    et.update_(et.Descent(0.1), As, grads, indexers)
    Eb, cb = wr.expanded_gradient(blk(2), wb, colptr_of(Lb), len(vb))
    Ef, cf = wr.expanded_gradient(blk(3), wf.reshape(-1), 1 + 3 * np.arange(B + 1), B * 3)
    exp_d = [blk(0)[np.repeat(np.arange(B), La)], blk(1), Eb[cb], Ef[cf]]
    exp_i = [va, Imat, vb[cb], Ifix.reshape(-1)[cf]]
    oracle.sgd_multi(hs, exp_d, exp_i, 0.1, [fused_update_path(A) for A in As])
    for A, h in zip(As, hs):
        assert same(host(A.data), h)
    # indexers are filled from the indices as before
    cum, mp = oracle.index_build(Ifix, ROWS)
    assert same(host(indexers[3].cumulative), cum) and same(host(indexers[3].map), mp)
    cum, mp = oracle.index_build(vb, ROWS)
    assert same(host(indexers[2].cumulative), cum)
    assert same(host(indexers[2].map), np.repeat(np.arange(B), Lb)[mp - 1] + 1)
    assert et.check_errors() == 0


# --- 12. rrule, the mean pullback, uncompress, refusals ------------------------------------------------

def test_rrule_weight_grad_mean_pullback_and_uncompress(oracle):
    rng = np.random.default_rng(14)
    B, D = 130, 32
    L = mix_lengths(B, rng)
    cp = colptr_of(L)
    values = rng.integers(1, 80, int(L.sum())).astype(np.int64)
    table = rng.standard_normal((ROWS, D)).astype(np.float32)
    w = rng.standard_normal(len(values) + 5).astype(np.float32)
    vals = np.concatenate([values, values[:5]])  # with a capacity tail
    A = et.SimpleEmbedding(dev(table), Static(D))
    W = et.WeightedIndices(ragged(vals, cp), dev(w), weight_grad=True)
    y, back = et.rrule(et.lookup, A, W)
    assert same(host(y), wr.forward(table, vals, cp, w)[0])
    delta = rng.standard_normal((B, D)).astype(np.float32)
    _, grad, dw = back(dev(delta))
    assert isinstance(grad, et.SparseEmbeddingUpdate) and grad.indices is W.indices
    assert grad.weights.data_ptr() == W.weights.data_ptr()
    et.update_(et.Descent(0.1), A, grad)
    # dw came from the table before the update
    ref, mag = wr.weight_grad_f64(table, delta, vals, cp)
    bound = wr.gamma(D + 1, 2.0 ** -24) * mag
    assert dw.shape == W.weights.shape
    assert (np.abs(host(dw) - ref) <= bound).all()
    after = host(A.data)
    assert not same(after, table)
    ref2, _ = wr.weight_grad_f64(after, delta, vals, cp)
    assert not (np.abs(ref2 - ref) <= bound).all()  # the updated table gives another dw
    # without weight_grad, and for an unweighted sum: NoTangent, the plain gradient
    _, g2, t2 = et.rrule(et.lookup, A, et.WeightedIndices(ragged(vals, cp), dev(w)))[1](dev(delta))
    assert isinstance(t2, et.NoTangent) and g2.weights is not None
    _, g3, t3 = et.rrule(et.lookup, A, et.WeightedIndices(ragged(vals, cp)))[1](dev(delta))
    assert isinstance(t3, et.NoTangent) and g3.weights is None

    # mean: the pullback stores 1 / len(bag) per entry; fed to the reference they reproduce
    # the updated table
    for idx, cpi, flat in ((ragged(vals, cp), cp, vals),
                           (dev(vals[:B * 3].reshape(B, 3)), 1 + 3 * np.arange(B + 1),
                            vals[:B * 3])):
        T = et.SimpleEmbedding(dev(table), Static(D))
        M = et.WeightedIndices(idx, mode="mean")
        ym, backm = et.rrule(et.lookup, T, M)
        assert same(host(ym), wr.forward(table, flat, cpi, mode="mean")[0])
        _, gm, tm = backm(dev(delta))
        assert isinstance(tm, et.NoTangent)
        wm = host(gm.weights)
        lens = np.diff(cpi)
        covered = np.repeat(np.arange(B), lens)
        assert wm.dtype == np.float32 and wm.shape == (len(flat),)
        assert np.allclose(wm[:len(covered)], 1.0 / lens[covered], rtol=1e-6)
        assert not wm[len(covered):].any()
        et.update_(et.Descent(0.1), T, gm)
        E, cov = wr.expanded_gradient(delta, wm, cpi, len(flat))
        reft = table.copy()
        oracle.sgd(reft, E[cov], flat[cov], 0.1, fused=True)
        assert same(host(T.data), reft)
        # uncompress scales by the weights
        dense = host(et.uncompress(gm, ROWS))
        wantd = np.zeros((ROWS, D), np.float64)
        np.add.at(wantd, flat[cov] - 1, E[cov].astype(np.float64))
        assert np.allclose(dense, wantd, rtol=1e-4, atol=1e-4)

    # refusals
    with pytest.raises(et.ArgumentError):
        et.update_(et.AdaGrad(0.1), A, grad)
    with pytest.raises(et.ArgumentError):
        et.PhasedUpdate([A], [grad])
    with pytest.raises(et.ArgumentError):
        et.update_(et.Descent(0.1), A, grad, exact=False)
    assert et.check_errors() == 0


# --- 13. graph capture: refill values / weights / colptr in place, replay another total --------------

def test_graph_capture_refill(oracle):
    from embtab.weighted import weight_grad

    rng = np.random.default_rng(15)
    B, D, CAP = 130, 128, 3000
    table = rng.standard_normal((ROWS, D)).astype(np.float32)
    delta = rng.standard_normal((B, D)).astype(np.float32)

    def inputs(mix):
        L = mix_lengths(B, rng) if mix else rng.integers(0, 6, B).astype(np.int64)
        v = rng.integers(1, ROWS + 1, int(L.sum())).astype(np.int64)
        assert len(v) <= CAP
        return L, v, rng.standard_normal(len(v)).astype(np.float32)

    vals = torch.ones(CAP, dtype=torch.int64, device=DEV)
    wts = torch.full((CAP,), float("nan"), device=DEV)
    colptr = torch.ones(B + 1, dtype=torch.int64, device=DEV)
    R = et.RaggedIndices(vals, colptr)
    W = et.WeightedIndices(R, wts)
    ddev = dev(delta)
    A = et.SimpleEmbedding(dev(table), Static(D))
    dst = torch.empty((B, D), device=DEV)
    dw = torch.empty(CAP, device=DEV)

    def fill(L, v, w):
        vals[:len(v)].copy_(dev(v))
        wts.fill_(float("nan"))
        wts[:len(w)].copy_(dev(w))
        colptr.copy_(dev(colptr_of(L)))

    def step(T, out, dwo):
        et.lookup_(out, T, W)
        weight_grad(T, ddev, R, out=dwo)
        et.update_(et.Descent(0.1), T, et.SparseEmbeddingUpdate(T.lookup_type, ddev, R, wts))

    L1, v1, w1 = inputs(True)
    fill(L1, v1, w1)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # one eager step first (workspaces), on a scratch table
        step(et.SimpleEmbedding(dev(table), Static(D)), torch.empty_like(dst),
             torch.empty_like(dw))
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step(A, dst, dw)
    L2, v2, w2 = inputs(False)
    assert 0 < len(v2) < len(v1)
    fill(L2, v2, w2)
    g.replay()
    torch.cuda.synchronize()
    # the eager result on the same inputs
    A2 = et.SimpleEmbedding(dev(table), Static(D))
    dst2, dw2 = torch.empty_like(dst), torch.empty_like(dw)
    step(A2, dst2, dw2)
    assert same(host(dst), host(dst2)) and same(host(dw), host(dw2))
    assert same(host(A.data), host(A2.data))
    cp2 = colptr_of(L2)
    wfull = host(wts)
    assert same(host(dst), wr.forward(table, host(vals), cp2, wfull, nnz=CAP)[0])
    E, cov = wr.expanded_gradient(delta, wfull, cp2, CAP)
    ref = table.copy()
    oracle.sgd(ref, E[cov], host(vals)[cov], 0.1, fused=True)
    assert same(host(A.data), ref)
    assert same(host(dw)[len(v2):], np.zeros(CAP - len(v2), np.float32))
    assert et.check_errors() == 0
