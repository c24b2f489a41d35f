"""Sparse AdaGrad over weighted and mean-pooled gradients on the GPU (et_weighted_adagrad
through ``et.AdaGrad`` / ``update_`` with a gradient that carries ``weights``).

The expected values are tests/test_gpu_adagrad.py's ``ref_step`` fed with the weighted
gradient sum of tests/weighted_adagrad_ref.py (the chunk rule of include/embtab.h: per chunk
``p = +0``, ``t = w_k * delta[bag(k)]``, ``p = p + t``, the partial sums added in chunk
order), compared with ``tobytes()`` equality.  The only tolerance is the row-wise bound
(``weighted_adagrad_ref.rowwise_bounds``), which tests/test_weighted_adagrad_host.py first
checks on the CPU for these very inputs.  Shapes and helpers are test_gpu_adagrad.py's: 300
columns; ``ragged_case`` (301 bags, a 40-entry uncovered head, a 600-entry tail, column 14
longer than a chunk with uncovered entries inside its list); ``make_indices`` (pool 4 x batch
1024 with columns of 1 / 255 / 256 / 257 / 513 / 2307 occurrences)."""
import ctypes

import numpy as np
import pytest
import torch

import embtab as et
import weighted_adagrad_ref as war
import weighted_ref as wr
from embtab import _lib
from embtab import update as upd
from embtab.tables import Static
from embtab.weighted import mean_weights, weight_grad
from test_gpu_adagrad import (B, CHUNK, EPS, ETA, FORCED, KINDS, P, R, ROW_CASES, make_indices,
                              padding_intact, ragged_case, wide_pair)
from test_gpu_ragged import ScatteredColumns, colptr_of, dev, host, mix_lengths, same

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def AdaGrad(*args, **kw):
    """The optimiser that takes weighted gradients (a default one refuses them)."""
    return et.AdaGrad(*args, weighted=True, **kw)


def test_default_optimiser_still_refuses_and_the_opt_in_is_the_only_difference():
    kind = KINDS["f32"]
    rng = np.random.default_rng(1000)
    L, values, colptr = ragged_case(rng)
    table = rng.standard_normal((R, 16)).astype(np.float32)
    delta = rng.standard_normal((len(L), 16)).astype(np.float32)
    w = war.case_weights(rng, values, colptr, np.float32)
    A = et.SimpleEmbedding(dev(table))
    for args in ((A, wgrad(kind, A, delta, values, colptr, w)),
                 ([A], [wgrad(kind, A, delta, values, colptr, w)])):
        with pytest.raises(et.ArgumentError, match="weighted=True"):
            et.update_(et.AdaGrad(ETA, EPS), *args)
    assert same(host(A.data), table)  # refused before anything ran
    # without weights both optimisers are the same update
    got = []
    for opt in (et.AdaGrad(ETA, EPS), AdaGrad(ETA, EPS)):
        T = et.SimpleEmbedding(dev(table))
        Rg = et.RaggedIndices(dev(values), dev(colptr))
        et.update_(opt, T, et.SparseEmbeddingUpdate(T.lookup_type, dev(delta), Rg))
        got.append((host(T.data), host(opt.state(T))))
    assert same(got[0][0], got[1][0]) and same(got[0][1], got[1][1])
    assert et.check_errors() == 0


def state_kind(kind):
    return KINDS["f64" if kind.C is np.float64 else "f32"]


def wgrad(kind, A, delta, values, colptr, weights):
    Rg = et.RaggedIndices(dev(values), dev(colptr))
    return et.SparseEmbeddingUpdate(A.lookup_type, kind.dev(delta), Rg, dev(weights))


def dense(A):
    if isinstance(A, ScatteredColumns):
        return A.dense()
    return host(A.to_dense() if isinstance(A, et.SplitEmbedding) else A.data)


# --- 1. the numpy reference, element-wise -----------------------------------------------------------

GEOMETRY = ([("f32", d) for d in (128, 16, 20, 1504, 7)] +
            [(n, d) for n in ("f64", "f16", "bf16") for d in (128, 20)])


@pytest.mark.parametrize("name,dim", GEOMETRY)
def test_reference_elementwise(name, dim):
    kind = KINDS[name]
    rng = np.random.default_rng(1100 + dim)
    table = kind.fromf(rng.standard_normal((R, dim)))
    state = rng.random((R, dim)).astype(kind.C)
    table0, state0 = table.copy(), state.copy()
    tw, tv = wide_pair(kind, table)
    sw, sv = wide_pair(state_kind(kind), state)
    A = et.SimpleEmbedding(tv)
    assert A.ld == dim + 8
    opt = AdaGrad(ETA, EPS)
    opt.set_state(A, sv)
    touched = set()
    for step in range(2):  # fresh indices, weights and gradients; the state is carried
        L, values, colptr = ragged_case(rng)
        delta = kind.fromf(rng.standard_normal((len(L), dim)))
        w = war.case_weights(rng, values, colptr, kind.C)
        assert np.isnan(w[:40]).all() and np.isnan(w[-600:]).all() and not np.isnan(w[40:-600]).any()
        et.update_(opt, A, wgrad(kind, A, delta, values, colptr, w), nontemporal=step == 0)
        lists, g_of = war.ref_step(kind, table, state, delta, values, colptr, w)
        assert len(lists[13]) > CHUNK + 40 and lists[13][0] == 0 and lists[13][-1] == 0
        assert any(c not in g_of for c in lists)  # a column that only uncovered entries hold
        touched |= set(g_of)
        assert same(host(tv), table), step
        assert same(host(sv), state), step
        assert padding_intact(tw, dim) and padding_intact(sw, dim)
    untouched = np.setdiff1d(np.arange(R), sorted(touched))
    assert len(untouched) >= 40
    assert same(host(tv)[untouched], table0[untouched])
    assert same(host(sv)[untouched], state0[untouched])
    assert not same(state, state0)
    assert et.check_errors() == 0


# --- 2. identity (a): every covered weight 1.0 --------------------------------------------------------

@pytest.mark.parametrize("rowwise", [False, True])
@pytest.mark.parametrize("dim", [128, 7])
def test_unit_weights_equal_the_unweighted_update(dim, rowwise):
    rng = np.random.default_rng(1200 + dim)
    table = rng.standard_normal((R, dim)).astype(np.float32)
    L, values, colptr = ragged_case(rng)
    I = make_indices(rng)
    for indices, nb, ones in (
            (lambda: et.RaggedIndices(dev(values), dev(colptr)), len(L), np.ones(len(values))),
            (lambda: dev(I), B, np.ones((B, P)))):
        delta = rng.standard_normal((nb, dim)).astype(np.float32)
        got = []
        for weights in (None, dev(ones.astype(np.float32))):
            A = et.SimpleEmbedding(dev(table))
            opt = AdaGrad(ETA, EPS, rowwise=rowwise, initial_accumulator_value=0.5)
            for step in range(2):
                et.update_(opt, A, et.SparseEmbeddingUpdate(A.lookup_type, dev(delta), indices(),
                                                            weights))
            got.append((host(A.data), host(opt.state(A))))
        assert same(got[0][0], got[1][0]) and same(got[0][1], got[1][1])
        assert not same(got[0][0], table)
    assert et.check_errors() == 0


# --- 3. identity (b): the expanded gradient -----------------------------------------------------------

@pytest.mark.parametrize("name", ["f32", "f64"])
@pytest.mark.parametrize("dim", [128, 7])
def test_equals_the_unweighted_update_of_the_expanded_gradient(name, dim):
    kind = KINDS[name]
    rng = np.random.default_rng(1300 + dim)
    L, values, colptr = ragged_case(rng, tail=1400)
    nnz = len(values)
    assert (values == 14).sum() > 2 * CHUNK  # column 14: more than two chunks
    table = kind.fromf(rng.standard_normal((R, dim)))
    delta = kind.fromf(rng.standard_normal((len(L), dim)))
    w = war.case_weights(rng, values, colptr, kind.C)
    E, covered = wr.expanded_gradient(delta, w, colptr, nnz)
    lo, hi = int(colptr[0]) - 1, int(colptr[-1]) - 1
    assert covered[lo:hi].all() and covered.sum() == hi - lo and lo == 40 and hi < nnz
    got = []
    for weighted in (True, False):
        A = et.SimpleEmbedding(kind.dev(table))
        opt = AdaGrad(ETA, EPS, initial_accumulator_value=0.25)
        if weighted:
            g = wgrad(kind, A, delta, values, colptr, w)
        else:  # every covered entry its own bag; head and tail stay uncovered
            own = np.arange(lo + 1, hi + 2, dtype=np.int64)
            g = et.SparseEmbeddingUpdate(A.lookup_type, dev(E[lo:hi]),
                                         et.RaggedIndices(dev(values), dev(own)))
        et.update_(opt, A, g)
        got.append((host(A.data), host(opt.state(A))))
    assert same(got[0][0], got[1][0]) and same(got[0][1], got[1][1])
    assert not same(got[0][0], table)
    assert et.check_errors() == 0


# --- 4. row-wise -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,dim", ROW_CASES)
def test_rowwise(name, dim):
    kind = KINDS[name]
    c = war.rowwise_case(name, dim, 0)
    table, state = c["table"], c["state"]
    A = et.SimpleEmbedding(kind.dev(table))
    opt = AdaGrad(ETA, EPS, rowwise=True)
    S = opt.state(A)
    assert S.shape == (R,) and S.dtype == (torch.float64 if name == "f64" else torch.float32)
    S.copy_(dev(state))
    for step in range(2):
        c = war.rowwise_case(name, dim, step)
        et.update_(opt, A, wgrad(kind, A, c["delta"], c["values"], c["colptr"], c["weights"]),
                   nontemporal=step == 0)
        got_t, got_s = host(A.data), host(S)
        rs, rw = war.rowwise_bounds(kind, table, state, c["g_of"], got_t, got_s)
        print(f"weighted rowwise GPU ratio {name} dim {dim} step {step}: state {rs:.3f} "
              f"table {rw:.3f}")
        assert rs <= 1.0 and rw <= 1.0, (step, rs, rw)
        table, state = got_t, got_s  # each step is judged alone, from what the GPU wrote
    assert et.check_errors() == 0


# --- 5. mean mode and weight_grad, end to end -----------------------------------------------------------

@pytest.mark.parametrize("dim", [128, 7])
def test_mean_mode_end_to_end(dim):
    kind = KINDS["f32"]
    rng = np.random.default_rng(1500 + dim)
    L, values, colptr = ragged_case(rng)
    table = rng.standard_normal((R, dim)).astype(np.float32)
    state = np.zeros((R, dim), np.float32)
    delta = rng.standard_normal((len(L), dim)).astype(np.float32)
    A = et.SimpleEmbedding(dev(table))
    W = et.WeightedIndices(et.RaggedIndices(dev(values), dev(colptr)), mode="mean")
    y, back = et.rrule(et.lookup, A, W)
    assert same(host(y), wr.forward(table, values, colptr, mode="mean")[0])
    _, grad, dw = back(dev(delta))
    assert isinstance(dw, et.NoTangent) and grad.weights is not None
    opt = AdaGrad(ETA, EPS)
    et.update_(opt, A, grad)
    w = host(grad.weights)  # as the binding rounded the reciprocals
    used = int(L.sum())
    assert (w[40:40 + used] > 0).all() and (w[40:40 + used] <= 1).all()
    assert (w[:40] == 0).all() and (w[40 + used:] == 0).all()
    war.ref_step(kind, table, state, delta, values, colptr, w)
    assert same(host(A.data), table) and same(host(opt.state(A)), state)
    assert et.check_errors() == 0


def test_weights_with_weight_grad_end_to_end():
    kind = KINDS["f32"]
    dim = 128
    rng = np.random.default_rng(1550)
    L, values, colptr = ragged_case(rng)
    table = rng.standard_normal((R, dim)).astype(np.float32)
    state = np.zeros((R, dim), np.float32)
    delta = rng.standard_normal((len(L), dim)).astype(np.float32)
    w = war.case_weights(rng, values, colptr, np.float32)
    A, A0 = et.SimpleEmbedding(dev(table)), et.SimpleEmbedding(dev(table))
    Rg = et.RaggedIndices(dev(values), dev(colptr))
    W = et.WeightedIndices(Rg, dev(w), weight_grad=True)
    y, back = et.rrule(et.lookup, A, W)
    _, grad, dw = back(dev(delta))
    opt = AdaGrad(ETA, EPS)
    et.update_(opt, A, grad)
    # dw comes from the table as it was before the update: the same call on an untouched copy
    assert same(host(dw), host(weight_grad(A0, dev(delta), Rg)))
    assert not same(host(dw), host(weight_grad(A, dev(delta), Rg)))
    war.ref_step(kind, table, state, delta, values, colptr, w)
    assert same(host(A.data), table) and same(host(opt.state(A)), state)
    assert et.check_errors() == 0


# --- 6. storage -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("store", ["split64", "colptr_vec", "colptr_generic"])
def test_storage(store):
    kind = KINDS["f32"]
    rng = np.random.default_rng(1600)
    dim = 10 if store == "colptr_generic" else 128
    table = rng.standard_normal((R, dim)).astype(np.float32)
    state = rng.random((R, dim)).astype(np.float32)
    if store == "split64":
        A = et.SplitEmbedding(dev(table), 64)
    else:
        A = ScatteredColumns(table, dim + (4 if store == "colptr_vec" else 3), rng)
    opt = AdaGrad(ETA, EPS)
    S = opt.state(A)
    assert S.is_contiguous() and S.shape == (R, dim)
    S.copy_(dev(state))
    for step in range(2):
        L, values, colptr = ragged_case(rng)
        delta = rng.standard_normal((len(L), dim)).astype(np.float32)
        w = war.case_weights(rng, values, colptr, np.float32)
        et.update_(opt, A, wgrad(kind, A, delta, values, colptr, w))
        war.ref_step(kind, table, state, delta, values, colptr, w)
        assert same(dense(A), table) and same(host(S), state), step
    assert et.check_errors() == 0


# --- 7. multi-table ---------------------------------------------------------------------------------------

def _as_weighted(d):
    """An AdaGradDesc as a WeightedAdaGradDesc with NULL weights."""
    if isinstance(d, _lib.WeightedAdaGradDesc):
        return d
    return _lib.WeightedAdaGradDesc(*[getattr(d, f[0]) for f in _lib.AdaGradDesc._fields_], None)


def _abi_call(opt, descs):
    L = _lib.load()
    arr = (_lib.WeightedAdaGradDesc * len(descs))(*descs)
    nb = ctypes.c_int64(0)
    _lib.check(L.et_weighted_adagrad_workspace_size(ctypes.addressof(arr), len(descs),
                                                    ctypes.byref(nb)))
    ws = torch.empty(nb.value, dtype=torch.uint8, device=DEV)
    _lib.check(L.et_weighted_adagrad(_lib.ET_F32, ctypes.addressof(arr), len(descs), opt.eta,
                                     opt.eps, _lib.ET_FLAG_NONTEMPORAL, ws.data_ptr(), ws.numel(),
                                     _lib.stream_handle(DEV)))
    torch.cuda.synchronize()


@pytest.mark.parametrize("k", [3, 4])  # prependrows: element-aligned, then 16-byte aligned
def test_multi_table_equals_single_calls(k):
    rng = np.random.default_rng(1700)
    dims = [128, 64, 20, 128, 8]
    hs = [rng.standard_normal((R, d)).astype(np.float32) for d in dims]
    Lr = mix_lengths(B, rng)
    vals = [rng.integers(1, R + 1, int(Lr.sum()) + 100).astype(np.int64) for _ in range(3)]
    for v in vals:
        v[:600] = 14  # a hot column: a bag of 300 among the lengths makes no chunk of its own
    cp = dev(colptr_of(Lr))
    rag = [et.RaggedIndices(dev(v), cp) for v in vals]
    I0, I3 = dev(make_indices(rng)), dev(make_indices(rng))
    w2 = torch.full((len(vals[1]),), float("nan"), device=DEV)
    w2[:int(Lr.sum())] = dev((0.25 + 1.75 * rng.random(int(Lr.sum()))).astype(np.float32))
    w3 = dev((0.25 + 1.75 * rng.random((B, P))).astype(np.float32))
    delta = dev(rng.standard_normal((B, k + sum(dims))).astype(np.float32))

    def build():
        As = [et.SimpleEmbedding(dev(hs[0])), et.SimpleEmbedding(dev(hs[1]), Static(64)),
              et.SimpleEmbedding(dev(hs[2])), et.SplitEmbedding(dev(hs[3]), 64),
              et.SimpleEmbedding(dev(hs[4]))]
        offs = np.cumsum([k] + dims)
        sl = [delta[:, offs[t]:offs[t + 1]] for t in range(5)]
        S = et.SparseEmbeddingUpdate
        grads = [S(As[0].lookup_type, sl[0], I0),                  # fixed pool, no weights
                 S(As[1].lookup_type, sl[1], rag[0]),              # ragged, no weights
                 S(As[2].lookup_type, sl[2], rag[1], w2),          # ragged, weights
                 S(As[3].lookup_type, sl[3], I3, w3),              # (B, P), weights
                 S(As[4].lookup_type, sl[4], rag[2], mean_weights(rag[2], torch.float32))]
        assert grads[1].delta.stride(0) == k + sum(dims)
        return As, grads, AdaGrad(ETA, EPS, initial_accumulator_value=0.1)

    As, grads, opt = build()
    Bs, grads1, opt1 = build()
    Cs, grads2, opt2 = build()
    for step in range(2):
        et.update_(opt, As, grads)
        for A, g in zip(Bs, grads1):
            et.update_(opt1, A, g)
        # at the ABI: all five kinds in one et_weighted_adagrad call
        descs = [upd._weighted_adagrad_desc(opt2, A, g) if g.weights is not None
                 else _as_weighted(upd._adagrad_desc(opt2, A, g)) for A, g in zip(Cs, grads2)]
        assert [d.weights is None for d in descs] == [True, True, False, False, False]
        assert [d.colptr is None for d in descs] == [True, False, False, False, False]
        _abi_call(opt2, descs)
    for t in range(5):
        for X, o in ((Bs, opt1), (Cs, opt2)):
            assert same(dense(As[t]), dense(X[t])), t
            assert same(host(opt.state(As[t])), host(o.state(X[t]))), t
        assert not same(dense(As[t]), hs[t])
    assert et.check_errors() == 0


# --- 8. out-of-range indices and colptr bounds -----------------------------------------------------------

@pytest.mark.parametrize("dim", [128, 7])
def test_out_of_range_is_counted_and_skipped(dim):
    kind = KINDS["f32"]
    rng = np.random.default_rng(1800)
    L, values, colptr = ragged_case(rng)
    nnz = len(values)
    used = np.arange(40, int(colptr[-1]) - 1)
    bad = rng.choice(used[values[used] >= 20], 6, replace=False)
    values[bad[:3]], values[bad[3:]] = 0, R + 1
    colptr = colptr.copy()
    colptr[-1] = nnz + 50  # the last bag now runs past the capacity: clamped to nnz, counted
    rg, clamped = wr.ranges(colptr, nnz)
    assert clamped == 1 and rg[-1][1] == nnz and rg[-1][1] - rg[-1][0] == 600
    w = war.case_weights(rng, values, colptr, np.float32)
    assert not np.isnan(w[-600:]).any()
    table = rng.standard_normal((R, dim)).astype(np.float32)
    state = rng.random((R, dim)).astype(np.float32)
    delta = rng.standard_normal((len(L), dim)).astype(np.float32)
    A = et.SimpleEmbedding(dev(table))
    opt = AdaGrad(ETA, EPS)
    opt.state(A).copy_(dev(state))
    et.check_errors()
    et.update_(opt, A, wgrad(kind, A, delta, values, colptr, w))
    assert et.check_errors() == 6 + clamped
    war.ref_step(kind, table, state, delta, values, colptr, w)
    assert same(host(A.data), table) and same(host(opt.state(A)), state)


# --- 9. graph capture ---------------------------------------------------------------------------------------

def test_graph_capture_refill():
    kind = KINDS["f32"]
    rng = np.random.default_rng(1900)
    dim, nb, CAP = 128, 301, 4000
    table = rng.standard_normal((R, dim)).astype(np.float32)
    vals = torch.ones(CAP, dtype=torch.int64, device=DEV)
    wts = torch.full((CAP,), float("nan"), device=DEV)
    colptr = torch.ones(nb + 1, dtype=torch.int64, device=DEV)
    ddev = torch.zeros((nb, dim), device=DEV)
    Rg = et.RaggedIndices(vals, colptr)
    W = et.WeightedIndices(Rg, wts)

    def fill():
        L, v, cp = ragged_case(rng)
        assert len(v) <= CAP
        delta = rng.standard_normal((nb, dim)).astype(np.float32)
        w = war.case_weights(rng, v, cp, np.float32)
        vals.fill_(1)
        wts.fill_(float("nan"))
        vals[:len(v)].copy_(dev(v))
        wts[:len(w)].copy_(dev(w))
        colptr.copy_(dev(cp))
        ddev.copy_(dev(delta))
        return delta

    def step(T, o, out):
        et.lookup_(out, T, W)
        et.update_(o, T, et.SparseEmbeddingUpdate(T.lookup_type, ddev, Rg, wts))

    fill()
    A = et.SimpleEmbedding(dev(table), Static(dim))
    opt = AdaGrad(ETA, EPS)
    opt.state(A)  # allocated before the capture
    dst = torch.empty((nb, dim), device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # one eager step first (workspaces), on a scratch table
        step(et.SimpleEmbedding(dev(table), Static(dim)), AdaGrad(ETA, EPS),
             torch.empty_like(dst))
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step(A, opt, dst)
    delta2 = fill()  # refill values, colptr, weights and the gradient in place, then replay
    g.replay()
    torch.cuda.synchronize()
    A2 = et.SimpleEmbedding(dev(table), Static(dim))
    opt2 = AdaGrad(ETA, EPS)
    dst2 = torch.empty_like(dst)
    step(A2, opt2, dst2)
    assert same(host(dst), host(dst2))
    assert same(host(A.data), host(A2.data)) and same(host(opt.state(A)), host(opt2.state(A2)))
    state = np.zeros((R, dim), np.float32)
    war.ref_step(kind, table, state, delta2, host(vals), host(colptr), host(wts))
    assert same(host(A.data), table) and same(host(opt.state(A)), state)
    assert et.check_errors() == 0
