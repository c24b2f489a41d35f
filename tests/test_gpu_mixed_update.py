"""Float32 tables updated from Float16 / BFloat16 gradients on the GPU (ET_FLAG_DELTA_F16 /
ET_FLAG_DELTA_BF16 through ``et.AdaGrad`` / ``et.Adam``) against the numpy models, bit for bit
(a NaN by position): table, state or moments, and step.

Shapes: 50-row tables whose last column is never indexed; 64 * 3 random occurrences and 600 of
the hot column 3 (three chunks: the combine pass runs), shuffled, with one out-of-range entry;
as 264 bags of pool 3, or as 200 ragged bags (empty ones among them) over the same values with
a capacity tail of 40 entries no bag covers."""
import copy

import numpy as np
import pytest
import torch

import embtab as et
from adam_ref import AdamModel, grad_sum, lists_fixed, lists_ragged

gpu = pytest.mark.gpu
DEV = torch.device("cuda:0")
R, P, HOT = 50, 3, 3
ADAM, ADA = dict(eta=0.01, beta=(0.9, 0.999), eps=1e-8), dict(eta=0.1, eps=1e-8)
GT = {"f16": torch.float16, "bf16": torch.bfloat16}


class AdaGradModel:
    """et_sparse_adagrad in numpy Float32: grad_sum, then the apply step of the header."""

    def __init__(self, table, eta, eps, rowwise=False):
        self.table, self.rowwise = table.clone(), rowwise
        self.s = np.zeros(table.shape[0] if rowwise else tuple(table.shape), np.float32)
        self.eta, self.eps = np.float32(eta), np.float32(eps)

    def update(self, delta, lists, feature_order=None):
        dC, w = delta.float().numpy(), self.table.numpy()  # w shares the table's memory
        for col, bags in lists.items():
            if not any(bags):
                continue
            g = grad_sum(dC, bags)
            if self.rowwise:
                ss = np.float32(0)
                for f in (range(len(g)) if feature_order is None else feature_order):
                    ss = ss + g[f] * g[f]
                s2 = self.s[col] + ss / np.float32(len(g))
            else:
                s2 = self.s[col] + g * g
            self.s[col] = s2
            w[col] = w[col] - (self.eta * g) / (np.sqrt(s2) + self.eps)


def normal(rng, shape, dtype):
    return torch.from_numpy(rng.standard_normal(shape)).to(dtype)


def eighths(rng, shape, dtype):  # sums and sums of squares are exact in Float32
    return torch.from_numpy(rng.integers(-4, 5, shape) / 8.0).to(dtype)


def special(rng, shape, dtype):  # the smallest subnormal, both zeros, +Inf and a NaN
    d = normal(rng, shape, dtype)
    d[:, 0], d[:, 1], d[::2, 1], d[5, 2], d[7, 3] = 2.0 ** -24, -0.0, 0.0, float("inf"), float("nan")
    return d


def make_index(rng, form, bad=True):
    flat = rng.permutation(np.concatenate([rng.integers(1, R, 64 * P), np.full(600, HOT)]))
    flat = flat.astype(np.int64)
    if bad:
        flat[31] = R + 1  # counted by check_errors, written nowhere
    if form == "fixed":
        I = flat.reshape(-1, P)
        return torch.from_numpy(I).to(DEV), I.shape[0], lists_fixed(I, R)
    cov = len(flat) - 40
    cuts = np.sort(rng.integers(0, cov + 1, 199))
    cuts[0], cuts[-1] = 0, cov  # the first and the last bag are empty
    colptr = 1 + np.concatenate([[0], cuts, [cov]]).astype(np.int64)
    idx = et.RaggedIndices(torch.from_numpy(flat).to(DEV), torch.from_numpy(colptr).to(DEV))
    return idx, 200, lists_ragged(flat, colptr, R)


def place(d, how):
    """``d`` on the device: contiguous, or as a view with an odd row stride, one element off a
    16-byte boundary, or inside a NaN-filled buffer (8 NaN columns either side, NaN rows)."""
    B, D = d.shape
    if how == "odd":
        big = torch.zeros((B, D + 3), dtype=d.dtype)
        v = big[:, :D]
    elif how == "offset":
        big = torch.zeros(B * D + 1, dtype=d.dtype)
        v = big[1:].view(B, D)
    elif how == "nan":
        big = torch.full((B + 2, D + 16), float("nan"), dtype=d.dtype)
        v = big[1:-1, 8:8 + D]
    else:
        return d.to(DEV)
    v.copy_(d)
    return big.to(DEV).as_strided(v.size(), v.stride(), v.storage_offset())


def same(got, want):
    got, want = got.cpu(), torch.as_tensor(want)
    nan = want.isnan()
    return (got.dtype == want.dtype == torch.float32 and torch.equal(got.isnan(), nan) and
            torch.equal(got[~nan].view(torch.int32), want[~nan].view(torch.int32)))


def check(opt, A, model):
    assert same(A.data, model.table)
    if isinstance(opt, et.Adam):
        m, v = opt.state(A)
        assert same(m, model.m) and same(v, model.v) and same(opt.step(A), model.step)
    else:
        assert same(opt.state(A), model.s)


def run(kind, rowwise, gtype, specs, gradient=None, steps=2):
    """Two carried steps of one call over the tables of ``specs`` (dim, index form, gradient
    placement), each checked against the model; returns the tables and the optimiser."""
    Opt, Model, hyper = (et.Adam, AdamModel, ADAM) if kind == "adam" else (et.AdaGrad, AdaGradModel, ADA)
    gradient = gradient or (eighths if rowwise else normal)
    rng = np.random.default_rng([kind == "adam", rowwise, gtype == "bf16", *[s[0] for s in specs]])
    tables = [normal(rng, (R, s[0]), torch.float32) for s in specs]
    As = [et.SimpleEmbedding(t.to(DEV)) for t in tables]
    opt, models = Opt(rowwise=rowwise, **hyper), [Model(t, rowwise=rowwise, **hyper) for t in tables]
    et.check_errors()
    for step in range(steps):
        grads = []
        for A, model, (dim, form, how) in zip(As, models, specs):
            idx, nb, lists = make_index(rng, form)
            d = gradient(rng, (nb, dim), GT[gtype])
            grads.append(et.SparseEmbeddingUpdate(A.lookup_type, place(d, how), idx))
            with np.errstate(all="ignore"):
                if rowwise:  # exact sums of squares: another order gives the same bits
                    other = copy.deepcopy(model)
                    other.update(d, lists, feature_order=rng.permutation(dim))
                model.update(d, lists)
            assert not rowwise or same(other.table, model.table)
        et.update_(opt, As, grads, nontemporal=step == 0)
        assert et.check_errors() == len(specs)
        for A, model in zip(As, models):
            check(opt, A, model)
    return As, opt, models


KIND = pytest.mark.parametrize("kind", ["adagrad", "adam"])
ROW = pytest.mark.parametrize("rowwise", [False, True])


@gpu
@KIND
@ROW
@pytest.mark.parametrize("gtype", ["f16", "bf16"])
@pytest.mark.parametrize("form", ["fixed", "ragged"])
@pytest.mark.parametrize("dim", [8, 40, 128, 520])  # one lane, masked 64, 4 records a wave, NV = 2
def test_vector_path_matches_the_model(kind, rowwise, gtype, form, dim):
    run(kind, rowwise, gtype, [(dim, form, "plain")])


@gpu
@KIND
@ROW
@pytest.mark.parametrize("specs", [[(12, "fixed", "plain")], [(128, "fixed", "odd")],
                                   [(128, "ragged", "offset")],
                                   [(128, "fixed", "plain"), (12, "ragged", "plain")]])
def test_generic_path_and_both_paths_in_one_call(kind, rowwise, specs):
    run(kind, rowwise, "bf16", specs)
    run(kind, rowwise, "f16", specs, steps=1)


@gpu
@KIND
@pytest.mark.parametrize("dim", [40, 520])
def test_views_in_nan_buffers(kind, dim):
    As, _, models = run(kind, False, "bf16", [(dim, "fixed", "nan")])
    assert not As[0].data.isnan().any() and not models[0].table.isnan().any()


@gpu
@KIND
@pytest.mark.parametrize("dim", [8, 12])  # the vector and the generic conversion
def test_special_values(kind, dim):
    _, _, models = run(kind, False, "f16", [(dim, "fixed", "plain")], gradient=special, steps=1)
    t = models[0].table  # the hot column met every bag: NaN and Inf; feature 0 only subnormals
    assert t[HOT - 1, 2:4].isnan().all() and not t[:, 0].isnan().any()


@gpu
@KIND
def test_equals_the_float32_path(kind):
    rng = np.random.default_rng(3)
    table = normal(rng, (R, 128), torch.float32)
    idx, nb, _ = make_index(rng, "fixed", bad=False)
    d = normal(rng, (nb, 128), torch.bfloat16).to(DEV)
    got = []
    for delta in (d, d.float()):
        A = et.SimpleEmbedding(table.to(DEV))
        opt = et.Adam(**ADAM) if kind == "adam" else et.AdaGrad(**ADA)
        et.update_(opt, A, et.SparseEmbeddingUpdate(A.lookup_type, delta, idx))
        state = opt.state(A)
        got.append([A.data, *(state if kind == "adam" else [state])])
    assert all(same(a, b.cpu()) for a, b in zip(*got)) and not same(got[0][0], table)


@gpu
def test_captured_bfloat16_step_replays():
    """One captured Adam step replayed twice, ``delta`` refilled in place, equals two eager steps
    and the model."""
    rng = np.random.default_rng(6)
    table = normal(rng, (R, 128), torch.float32)
    idx, nb, lists = make_index(rng, "fixed", bad=False)
    fills = [normal(rng, (nb, 128), torch.bfloat16) for _ in range(2)]
    model, ddev = AdamModel(table, **ADAM), fills[0].to(DEV)
    As = [et.SimpleEmbedding(table.to(DEV)) for _ in range(3)]  # scratch, eager, captured
    opts = [et.Adam(**ADAM) for _ in As]
    grad = lambda A: et.SparseEmbeddingUpdate(A.lookup_type, ddev, idx)
    opts[2].state(As[2]), opts[2].step(As[2])  # allocated before the capture
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # one eager step first, on the scratch table
        et.update_(opts[0], As[0], grad(As[0]))
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        et.update_(opts[2], As[2], grad(As[2]))
    for d in fills:
        ddev.copy_(d.to(DEV))
        et.update_(opts[1], As[1], grad(As[1]))
        g.replay()
        model.update(d, lists)
        check(opts[1], As[1], model)
        check(opts[2], As[2], model)
    assert et.check_errors() == 0
