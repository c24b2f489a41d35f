"""Sparse Adam over weighted and mean-pooled gradients on the GPU (et_weighted_adam through
``et.Adam(weighted=True)`` / ``update_``) against tests/adam_ref.py's AdamModel fed with the
expanded gradient of tests/weighted_adam_ref.py, bit for bit (``torch.equal`` on table, m, v
and step).

The ragged case (37-row tables, the last column never indexed): 240 entries in front of the
first bag and a capacity tail, both naming the hot column 3; 300 one-entry bags that hold the
hot column, so its list is longer than two chunks with covered entries in three; a column
that only the tail names; one out-of-range index; NaN weights wherever no bag covers the entry;
the gradient a view inside a NaN-filled buffer."""
import numpy as np
import pytest
import torch

import embtab as et
from adam_ref import CHUNK, lists_fixed
from test_gpu_adam import DEV, DIMS, HOT, HYPER, R, TYPES, check, eighths, normal
from weighted_adam_ref import AdamModel, expanded

pytestmark = pytest.mark.gpu
NB, CAP, HEAD, ZC = 341, 1070, 240, 5  # bags, capacity, uncovered head, the weight-0 column


def ragged_case(rng, C, draw=None, bad=True, zero_col=False):
    """(values, colptr, weights) of the case in the module docstring, always CAP entries and
    NB bags.  ``draw(rng, n)`` gives the covered weights (default: N(0, 1) with every seventh
    exactly 0); ``zero_col``: every covered entry of column ZC weighs exactly 0."""
    L = np.concatenate([[0], rng.integers(0, 13, 39), np.ones(300, np.int64), [0]])
    colptr = (HEAD + 1 + np.concatenate([[0], np.cumsum(L)])).astype(np.int64)
    lo, hi = HEAD, int(colptr[-1]) - 1
    values = rng.integers(1, R - 1, CAP).astype(np.int64)
    values[:HEAD] = HOT
    values[hi - 300:hi] = HOT
    values[hi::5], values[-3:] = HOT, R - 1  # the tail: the hot column, and a column of its own
    values[lo + 1:lo + 4] = ZC
    if bad:
        values[lo + 7] = R + 1  # counted by check_errors, written nowhere
    w = np.full(CAP, np.nan, C)
    if draw is None:
        w[lo:hi] = rng.standard_normal(hi - lo)
        w[lo:hi:7] = 0
    else:
        w[lo:hi] = draw(rng, hi - lo)
    if zero_col:
        w[lo:hi][values[lo:hi] == ZC] = 0
    assert CAP - hi >= 50 and (values == R).sum() == 0
    return values, colptr, w


def exact_weights(rng, n):
    return rng.choice([-1.0, 0.0, 0.5, 1.0], n)


def nan_view(delta):
    """The gradient as a view inside a NaN-filled device buffer (16-byte aligned rows)."""
    big = torch.full((delta.shape[0] + 2, delta.shape[1] + 4), float("nan"), dtype=delta.dtype,
                     device=DEV)
    big[1:-1, :delta.shape[1]] = delta.to(DEV)
    return big[1:-1, :delta.shape[1]]


def wgrad(A, delta, values, colptr, w):
    Rg = et.RaggedIndices(torch.from_numpy(values).to(DEV), torch.from_numpy(colptr).to(DEV))
    return et.SparseEmbeddingUpdate(A.lookup_type, nan_view(delta), Rg,
                                    None if w is None else torch.from_numpy(w).to(DEV))


def model_step(model, delta, values, colptr, w, rng=None):
    """One model step; with ``rng`` (row-wise, exact sums of squares) the model must give the
    same bits with a permuted feature order."""
    E, lists = expanded(delta, values, colptr, w, R)
    if rng is not None:
        other = AdamModel(model.table, rowwise=True, **HYPER)
        other.m, other.v, other.step = model.m.copy(), model.v.copy(), model.step.copy()
        other.update(E, lists, feature_order=rng.permutation(E.shape[1]))
    model.update(E, lists)
    if rng is not None:
        assert torch.equal(other.table, model.table) and np.array_equal(other.v, model.v)
    return lists


def ragged_run(name, dim, rowwise):
    dtype = TYPES[name]
    C = np.float64 if name == "f64" else np.float32
    rng = np.random.default_rng([dim, rowwise, sorted(TYPES).index(name), 22])
    gradient, draw = (eighths, exact_weights) if rowwise else (normal, None)
    table = normal(rng, (R, dim), dtype)
    A = et.SimpleEmbedding(table.to(DEV))
    opt = et.Adam(rowwise=rowwise, weighted=True, **HYPER)
    model = AdamModel(table, rowwise=rowwise, **HYPER)
    et.check_errors()
    for step in range(2):  # the moments and the step are carried
        values, colptr, w = ragged_case(rng, C, draw, zero_col=step == 1)
        delta = gradient(rng, (NB, dim), dtype)
        before = model.m[ZC - 1].copy(), model.v[ZC - 1].copy(), model.table[ZC - 1].clone()
        et.update_(opt, A, wgrad(A, delta, values, colptr, w), nontemporal=step == 0)
        lists = model_step(model, delta, values, colptr, w, rng if rowwise else None)
        hot = lists[HOT - 1]
        assert len(hot) > 2 * CHUNK and not any(lists[R - 2])
        assert sum(any(hot[c:c + CHUNK]) for c in range(0, len(hot), CHUNK)) >= 3
        assert et.check_errors() == 1
        check(opt, A, model)
    # step 1 reached column ZC through weight-0 entries only: its moments and row were written
    assert before[0].any() and not np.array_equal(model.m[ZC - 1], before[0])
    assert not np.array_equal(model.v[ZC - 1], before[1])
    assert not torch.equal(model.table[ZC - 1], before[2])
    assert not model.m[R - 1].any() and not model.m[R - 2].any() and model.m[HOT - 1].any()


@pytest.mark.parametrize("name,dim", [("f32", d) for d in DIMS] +
                         [(n, d) for n in ("f64", "f16", "bf16") for d in (12, 128)])
def test_elementwise(name, dim):
    ragged_run(name, dim, False)


@pytest.mark.parametrize("dim", DIMS)
def test_rowwise(dim):
    """Gradients in eighths, weights from {-1, 0, 0.5, 1}: every product, gradient sum and sum of
    squares is exact in Float32 (over 200 seeds of this case at dim 512 the integer sum of squares,
    in units of 1/256, peaks at 2.9e6, below 2^24), so its order cannot matter; ``model_step``
    asserts that on the model with a permuted feature order."""
    ragged_run("f32", dim, True)


def fixed_indices(rng, P=4):
    I = np.concatenate([rng.integers(1, R, 64 * P), np.full(600, HOT)])
    return rng.permutation(I).reshape(-1, P).astype(np.int64)


@pytest.mark.parametrize("rowwise", [False, True])
def test_unit_weights_and_mean_mode(rowwise):
    """Consequence (a): weights all 1.0 (NaN where no bag covers) equal ``et.Adam()`` without
    weights on the same ragged index.  Consequence (c): the pullback of a mean-pooled lookup over
    a fixed-pool (B, 4) index equals the model with w = 1 / 4."""
    rng = np.random.default_rng([31, rowwise])
    gradient = eighths if rowwise else normal
    for dim in (128, 6):
        table = normal(rng, (R, dim), torch.float32)
        values, colptr, w = ragged_case(rng, np.float32, lambda r, n: np.ones(n), bad=False)
        delta = gradient(rng, (NB, dim), torch.float32)
        got = []
        for weights in (w, None):
            A = et.SimpleEmbedding(table.to(DEV))
            opt = et.Adam(rowwise=rowwise, weighted=weights is not None, **HYPER)
            for _ in range(2):
                et.update_(opt, A, wgrad(A, delta, values, colptr, weights))
            got.append([A.data, *opt.state(A), opt.step(A)])
        assert all(torch.equal(a, b) for a, b in zip(*got))
        assert not torch.equal(got[0][0].cpu(), table)

        I = fixed_indices(rng)
        A = et.SimpleEmbedding(table.to(DEV))
        opt = et.Adam(rowwise=rowwise, weighted=True, **HYPER)
        model = AdamModel(table, rowwise=rowwise, **HYPER)
        delta = gradient(rng, (I.shape[0], dim), torch.float32)
        W = et.WeightedIndices(torch.from_numpy(I).to(DEV), mode="mean")
        _, back = et.rrule(et.lookup, A, W)
        grad = back(delta.to(DEV))[1]
        w = np.full(I.size, np.float32(1) / np.float32(4))
        assert torch.equal(grad.weights.cpu(), torch.from_numpy(w))
        et.update_(opt, A, grad)
        model_step(model, delta, I.reshape(-1), 1 + 4 * np.arange(I.shape[0] + 1), w,
                   rng if rowwise else None)
        check(opt, A, model)
    assert et.check_errors() == 0


@pytest.mark.parametrize("dims", [(128, 12), (6, 128)])
@pytest.mark.parametrize("rowwise", [False, True])
def test_mixed_call_eager_and_captured(dims, rowwise):
    """One call with an unweighted fixed-pool SplitEmbedding, a weighted ragged table and a table
    with no bags (it keeps table, moments and step).  The call is captured once and replayed
    three times with indices, weights and gradients refilled in place: equal to three eager
    calls and to the model."""
    rng = np.random.default_rng([41, dims[0], rowwise])
    gradient, draw = (eighths, exact_weights) if rowwise else (normal, None)
    tables = [normal(rng, (R, d), torch.float32) for d in (*dims, 16)]
    models = [AdamModel(t, rowwise=rowwise, **HYPER) for t in tables]
    I = torch.zeros((214, 4), dtype=torch.int64, device=DEV)
    vals = torch.ones(CAP, dtype=torch.int64, device=DEV)
    cp = torch.ones(NB + 1, dtype=torch.int64, device=DEV)
    wts = torch.full((CAP,), float("nan"), device=DEV)
    d0, d1 = torch.zeros((214, dims[0]), device=DEV), nan_view(torch.zeros((NB, dims[1])))
    idx = [I, et.RaggedIndices(vals, cp), torch.empty((0, 4), dtype=torch.int64, device=DEV)]
    deltas, weights = [d0, d1, torch.empty((0, 16), device=DEV)], [None, wts, None]

    def fill():
        host = fixed_indices(rng), gradient(rng, (214, dims[0]), torch.float32), *ragged_case(
            rng, np.float32, draw, bad=False), gradient(rng, (NB, dims[1]), torch.float32)
        for dst, src in zip((I, d0, vals, cp, wts, d1), host):
            dst.copy_(torch.as_tensor(src).to(DEV))
        return host

    def build():
        As = [et.SplitEmbedding(tables[0].to(DEV), 16), et.SimpleEmbedding(tables[1].to(DEV)),
              et.SimpleEmbedding(tables[2].to(DEV))]
        opt = et.Adam(rowwise=rowwise, weighted=True, **HYPER)
        for A in As:
            opt.state(A), opt.step(A)  # allocated before the capture
        grads = [et.SparseEmbeddingUpdate(A.lookup_type, d, i, w)
                 for A, d, i, w in zip(As, deltas, idx, weights)]
        return As, opt, grads

    fill()
    (As, opt, grads), (Gs, gopt, ggrads), (Ts, topt, tgrads) = build(), build(), build()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # one eager step first (workspaces), on scratch tables
        et.update_(topt, Ts, tgrads)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        et.update_(gopt, Gs, ggrads)
    assert (gopt.step(Gs[1]) == 1).all()  # a capture runs nothing
    for _ in range(3):
        Ih, d0h, values, colptr, w, d1h = fill()
        et.update_(opt, As, grads)
        g.replay()
        models[0].update(d0h, lists_fixed(Ih, R))
        model_step(models[1], d1h, values, colptr, w, rng if rowwise else None)
        for Xs, o in ((As, opt), (Gs, gopt)):
            for A, model in zip(Xs, models):
                check(o, A, model)
    assert not models[2].m.any() and (models[2].step == 1).all()
    assert et.check_errors() == 0
