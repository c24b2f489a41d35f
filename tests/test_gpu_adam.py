"""Sparse Adam on the GPU (et_sparse_adam through ``et.Adam`` / ``update_``) against the numpy
model of tests/adam_ref.py, bit for bit (``torch.equal`` on table, m, v and step).

Shapes: 37-row tables whose last column is never indexed; a fixed-pool index of pool 5 made of
64 random bags and 120 bags that hold only the hot column 3 (64 bags of pool 5 cannot hold the
600 occurrences the hot column needs for three chunks and the combine pass), shuffled
together, with one out-of-range entry."""
import numpy as np
import pytest
import torch

import embtab as et
from adam_ref import CHUNK, AdamModel, lists_fixed, lists_ragged

gpu = pytest.mark.gpu
DEV = torch.device("cuda:0")
R, P, HOT = 37, 5, 3
HYPER = dict(eta=0.01, beta=(0.9, 0.999), eps=1e-8)
TYPES = {"f32": torch.float32, "f64": torch.float64, "f16": torch.float16,
         "bf16": torch.bfloat16}
DIMS = [4, 12, 128, 512, 6]  # one lane per group, masked 16, two groups a wave, NV = 2, generic


def fixed_indices(rng, bad=True):
    I = np.concatenate([rng.integers(1, R, 64 * P), np.full(600, HOT)])
    I = rng.permutation(I).reshape(-1, P).astype(np.int64)
    if bad:
        I[11, 2] = R + 1  # counted by check_errors, written nowhere
    assert (I == R).sum() == 0 and 2 * CHUNK < (I == HOT).sum()
    return I


def normal(rng, shape, dtype):
    return torch.from_numpy(rng.standard_normal(shape)).to(dtype)


def eighths(rng, shape, dtype):
    return torch.from_numpy(rng.integers(-4, 5, shape) / 8.0).to(dtype)


def dense(A):
    return (A.to_dense() if isinstance(A, et.SplitEmbedding) else A.data).cpu()


def check(opt, A, model):
    m, v = opt.state(A)
    assert torch.equal(dense(A), model.table)
    assert torch.equal(m.cpu(), torch.from_numpy(model.m))
    assert torch.equal(v.cpu(), torch.from_numpy(model.v))
    assert torch.equal(opt.step(A).cpu(), torch.from_numpy(model.step))


def fixed_case(name, dim, rowwise, gradient, steps=2):
    dtype = TYPES[name]
    rng = np.random.default_rng([dim, rowwise, sorted(TYPES).index(name)])
    table = normal(rng, (R, dim), dtype)
    A = et.SimpleEmbedding(table.to(DEV))
    opt = et.Adam(rowwise=rowwise, **HYPER)
    model = AdamModel(table, rowwise=rowwise, **HYPER)
    et.check_errors()
    for step in range(steps):  # the moments and the step are carried
        I = fixed_indices(rng)
        delta = gradient(rng, (I.shape[0], dim), dtype)
        et.update_(opt, A, et.SparseEmbeddingUpdate(A.lookup_type, delta.to(DEV),
                                                    torch.from_numpy(I).to(DEV)),
                   nontemporal=step == 0)
        lists = lists_fixed(I, R)
        if rowwise:  # the sum of squares is exact for these inputs: any order, the same bits
            other = AdamModel(model.table, rowwise=True, **HYPER)
            other.m, other.v, other.step = model.m.copy(), model.v.copy(), model.step.copy()
            other.update(delta, lists, feature_order=rng.permutation(dim))
        model.update(delta, lists)
        if rowwise:
            assert torch.equal(other.table, model.table) and np.array_equal(other.v, model.v)
        assert et.check_errors() == 1
        check(opt, A, model)
    assert not model.m[R - 1].any() and model.m[HOT - 1].any()  # never indexed / the hot column


@gpu
@pytest.mark.parametrize("name,dim", [("f32", d) for d in DIMS] +
                         [(n, d) for n in ("f64", "f16", "bf16") for d in (12, 128)])
def test_elementwise(name, dim):
    fixed_case(name, dim, False, normal)


@gpu
@pytest.mark.parametrize("dim", DIMS)
def test_rowwise(dim):
    fixed_case("f32", dim, True, eighths)


@gpu
@pytest.mark.parametrize("dims", [(128, 12), (6, 128)])
@pytest.mark.parametrize("rowwise", [False, True])
def test_ragged_and_fixed_in_one_call(dims, rowwise):
    """A fixed-pool SplitEmbedding and a ragged table in one call, and a third table with no
    bags: its table, moments and step stay as they are.  The ragged index has 240 entries in
    front of the first bag and a capacity tail (colptr ends before nnz) that hold the hot column
    and a column no bag covers; its gradient is a view inside a NaN-filled buffer."""
    rng = np.random.default_rng([7, dims[0], rowwise])
    gradient = eighths if rowwise else normal
    tables = [normal(rng, (R, d), torch.float32) for d in (*dims, 16)]
    As = [et.SplitEmbedding(tables[0].to(DEV), 16), et.SimpleEmbedding(tables[1].to(DEV)),
          et.SimpleEmbedding(tables[2].to(DEV))]
    opt = et.Adam(rowwise=rowwise, **HYPER)
    models = [AdamModel(t, rowwise=rowwise, **HYPER) for t in tables]
    L = rng.integers(0, 13, 40)
    L[[0, -1]], L[17] = 0, 40  # a bag of 40 entries that holds the hot column only
    colptr = (241 + np.concatenate([[0], np.cumsum(L)])).astype(np.int64)
    values = rng.integers(1, R - 1, 240 + int(L.sum()) + 50).astype(np.int64)
    values[:240] = HOT  # in front of the first bag: no bag covers them, they keep their places
    values[colptr[17] - 1:colptr[18] - 1] = HOT
    values[-50::5], values[-3:] = HOT, R - 1  # the tail: the hot column, and a column of its own
    lists = lists_ragged(values, colptr, R)
    assert len(lists[HOT - 1]) > CHUNK + 20 and not any(lists[R - 2])
    I = fixed_indices(rng, bad=False)
    big = torch.full((len(L) + 2, dims[1] + 4), float("nan"))
    big[1:-1, :dims[1]] = gradient(rng, (len(L), dims[1]), torch.float32)
    deltas = [gradient(rng, (I.shape[0], dims[0]), torch.float32), big[1:-1, :dims[1]],
              torch.empty((0, 16))]
    idx = [torch.from_numpy(I).to(DEV),
           et.RaggedIndices(torch.from_numpy(values).to(DEV), torch.from_numpy(colptr).to(DEV)),
           torch.empty((0, P), dtype=torch.int64, device=DEV)]
    big = big.to(DEV)
    dev_deltas = [deltas[0].to(DEV), big[1:-1, :dims[1]], deltas[2].to(DEV)]
    for A in As:
        opt.state(A), opt.step(A)
    et.update_(opt, As, [et.SparseEmbeddingUpdate(A.lookup_type, d, i)
                         for A, d, i in zip(As, dev_deltas, idx)])
    models[0].update(deltas[0], lists_fixed(I, R))
    if rowwise:  # exact sums of squares: the model gives the same bits in another order
        other = AdamModel(tables[1], rowwise=True, **HYPER)
        other.update(deltas[1], lists, feature_order=rng.permutation(dims[1]))
    models[1].update(deltas[1], lists)
    assert not rowwise or torch.equal(other.table, models[1].table)
    for A, model in zip(As, models):
        check(opt, A, model)
    assert not models[2].m.any() and (models[2].step == 1).all()
    assert et.check_errors() == 0


@gpu
@pytest.mark.parametrize("rowwise", [False, True])
def test_step_state_eager_and_captured(rowwise):
    """Three eager steps equal three model steps, and one captured update_ replayed three
    times (gradients and indices refilled in place) equals them: the step state is advanced on
    the device, so a replay advances it as an eager call does."""
    dim = 128
    rng = np.random.default_rng([9, rowwise])
    gradient = eighths if rowwise else normal
    table = normal(rng, (R, dim), torch.float32)
    fills = [(fixed_indices(rng, bad=False), None) for _ in range(3)]
    fills = [(I, gradient(rng, (I.shape[0], dim), torch.float32)) for I, _ in fills]
    model = AdamModel(table, rowwise=rowwise, **HYPER)
    Idev = torch.from_numpy(fills[0][0]).to(DEV)
    ddev = fills[0][1].to(DEV)
    grad = lambda T: et.SparseEmbeddingUpdate(T.lookup_type, ddev, Idev)
    A, A2 = et.SimpleEmbedding(table.to(DEV)), et.SimpleEmbedding(table.to(DEV))
    opt, opt2 = et.Adam(rowwise=rowwise, **HYPER), et.Adam(rowwise=rowwise, **HYPER)
    opt2.state(A2), opt2.step(A2)  # allocated before the capture
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # one eager step first, on a scratch table
        T = et.SimpleEmbedding(table.to(DEV))
        et.update_(et.Adam(rowwise=rowwise, **HYPER), T, grad(T))
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        et.update_(opt2, A2, grad(A2))
    assert (opt2.step(A2) == 1).all()  # a capture runs nothing
    for I, delta in fills:
        Idev.copy_(torch.from_numpy(I).to(DEV))
        ddev.copy_(delta.to(DEV))
        et.update_(opt, A, grad(A))
        g.replay()
        model.update(delta, lists_fixed(I, R))
        check(opt, A, model)
        check(opt2, A2, model)
    C = np.float32
    p = np.ones(2, C)
    for _ in range(3):  # the running products, not a power
        p = p * np.array(HYPER["beta"], C)
    assert torch.equal(opt2.step(A2).cpu(), torch.from_numpy(p))
    assert et.check_errors() == 0
