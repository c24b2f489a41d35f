"""Weighted and mean-pooled bags over quantised tables on the GPU, byte for byte against the
numpy restatements: weighted_ref.forward on the decoded Float32 table, quant_ref.store for the
16-bit outputs.  R = 300 rows, B = 65 bags (more than one workgroup of the D = 128 geometry and
a partial group).  Ragged lengths cycle 0, 1, 3, 7, 8, 9, 17, 20, 33: every tail of the
8 / 4 / 2 / 1 ladder, more than one chunk at 8 and at 16 slots, empty first and last bags."""
import numpy as np
import pytest
import torch

import quant_ref as qr
import test_gpu_fp8 as tf
import test_gpu_mx4 as tm
import test_gpu_quant as tq
import weighted_ref as wr

pytestmark = pytest.mark.gpu

et = pytest.importorskip("embtab")

DEV, R, dev, raw = tq.DEV, tq.R, tq.dev, tq.raw
B, PAD = 65, 8
# format, bits, dim, ld_bytes: the kernel path
CASES = [("int", 8, 128, None),    # 8 lanes a bag
         ("int", 8, 96, None),     # a masked group
         ("int", 8, 256, None),    # 16 lanes, chunks of 16
         ("int", 8, 20, 24),       # generic
         ("int", 4, 32, None),     # 1 lane a bag, 8 slots a lane
         ("int", 4, 128, None),
         ("e4m3", 8, 48, None),    # a masked group of 4
         ("e5m2", 8, 128, None),
         ("mxfp4", 4, 128, None),
         ("mxfp4", 4, 96, 52)]     # generic
VECTOR = [c for c in CASES if c[2] in (128, 48)]  # one vector case per format


def table(fmt, bits, dim, ld, split):
    """(the table taking weighted indices, the same table without the flag, its decoded rows)."""
    if fmt == "int":
        Q, T = tq.table(bits, dim, split, 0, ld)
    elif fmt == "mxfp4":
        Q, T = tm.table(dim, split, ld)  # row 1 is NaN
    else:
        Q, T = tf.table(fmt, dim, split)
    return Q.accept_weighted(), Q, T


_BAGS = {}


def bags(seed=0):
    """(values, colptr, weights) on the host, built once: rows 2..R, an out-of-range index
    under a negative weight in a bag of three and one under a positive weight in the bag of 33,
    then PAD entries no bag covers (index R + 1, weight NaN)."""
    if seed not in _BAGS:
        rng = np.random.default_rng(seed)
        L = np.resize(np.array([0, 1, 3, 7, 8, 9, 17, 20, 33], np.int64), B)
        L[-1] = 0
        cp = wr.colptr_of(L)
        n = int(L.sum())
        v = np.concatenate([rng.integers(2, R + 1, n), np.full(PAD, R + 1)]).astype(np.int64)
        w = np.concatenate([rng.standard_normal(n), np.full(PAD, np.nan)]).astype(np.float32)
        assert (w[:n] < 0).any() and L[2] == 3 and L[8] == 33
        p3, p33 = int(cp[2]), int(cp[8]) + 16  # 0-based entries of bags 2 and 8
        v[[p3, p33]] = R + 1
        w[p3], w[p33] = -abs(w[p3]), abs(w[p33])
        _BAGS[seed] = (v, cp, w)
    return _BAGS[seed]


def windex(v, cp, w=None, mode="sum"):
    return et.WeightedIndices(et.RaggedIndices(dev(v), dev(cp)), None if w is None else dev(w),
                              mode=mode)


@pytest.mark.parametrize("split", (False, True))
@pytest.mark.parametrize("fmt,bits,dim,ld", CASES)
def test_weighted_and_mean_bags(fmt, bits, dim, ld, split):
    A, Q, T = table(fmt, bits, dim, ld, split)
    S = et.SimpleEmbedding(A.dequantize())
    v, cp, w = bags()
    et.check_errors()
    want, oob = wr.forward(T, v, cp, w, nnz=len(v))
    assert oob == 2 and np.isfinite(want).all() and not want[0].any() and not want[-1].any()
    for X in (A, S):  # the new kernel, and the float weighted kernel on the decoded table
        assert raw(et.lookup(X, windex(v, cp, w))) == want.tobytes()
        assert et.check_errors() == oob
    # no weights, and every weight 1.0: the existing unweighted kernel, bit for bit
    plain = raw(et.lookup(Q, et.RaggedIndices(dev(v), dev(cp))))
    assert raw(et.lookup(A, windex(v, cp))) == plain == wr.forward(T, v, cp, nnz=len(v))[0].tobytes()
    assert raw(et.lookup(A, windex(v, cp, np.ones_like(w)))) == plain
    # mean: bag 2 has three entries, one of them out of range (1/3 is inexact)
    want, _ = wr.forward(T, v, cp, mode="mean", nnz=len(v))
    got = et.lookup(A, windex(v, cp, mode="mean"))
    assert raw(got) == want.tobytes() and raw(got[0]) == bytes(4 * dim)
    assert et.check_errors() == 4 * oob


@pytest.mark.parametrize("P", (1, 8, 20))
def test_fixed_pool_is_its_ragged_form(P):
    A, _, T = table("int", 8, 128, None, False)
    rng = np.random.default_rng(P)
    idx = rng.integers(1, R + 1, (B, P)).astype(np.int64)
    w = rng.standard_normal((B, P)).astype(np.float32)
    cp = 1 + P * np.arange(B + 1, dtype=np.int64)
    want, _ = wr.forward(T, idx.reshape(-1), cp, w.reshape(-1))
    assert raw(et.lookup(A, et.WeightedIndices(dev(idx), dev(w)))) == want.tobytes()
    assert raw(et.lookup(A, windex(idx.reshape(-1), cp, w.reshape(-1)))) == want.tobytes()
    assert et.check_errors() == 0


@pytest.mark.parametrize("fmt,bits,dim,ld", VECTOR)
def test_sixteen_bit_destinations_round_once(fmt, bits, dim, ld):
    """Behind three prepended rows: the unaligned store path."""
    A, _, T = table(fmt, bits, dim, ld, False)
    v, cp, w = bags()
    for X, mode in ((windex(v, cp, w), "sum"), (windex(v, cp, mode="mean"), "mean")):
        acc, _ = wr.forward(T, v, cp, w if mode == "sum" else None, mode=mode, nnz=len(v))
        for name, dt in tq.OUTS:
            dst = torch.full((B, 3 + dim), -3.0, dtype=dt, device=DEV)
            et.maplookup_(et.PreallocationStrategy(3), dst, [A], [X])
            want = qr.store(np.full((B, 3 + dim), -3.0, np.float32), name)
            want[:, 3:] = qr.store(acc, name)
            assert raw(dst) == want.tobytes(), (mode, name)
    et.check_errors()


@pytest.mark.parametrize("k", (0, 3))
def test_one_entry_bag_rounds_twice(k):
    """v = 3 and w just above 1 + 2^-10 / 3: the exact product lies above a Float16 tie, its
    Float32 rounding on the tie.  The contract rounds to Float32, then to Float16."""
    w = np.float32(1 + 2731 * 2.0 ** -23)  # 2^13 / 3 = 2730.67 units of 2^-23
    assert float(np.nextafter(w, np.float32(0))) < 1 + 2.0 ** -10 / 3 < float(w)
    exact, tie = float(w) * 3.0, 3 + 2.0 ** -10  # the product is exact in Float64
    assert exact > tie and np.float32(exact) == np.float32(tie)
    assert np.float16(np.float32(exact)) == 3 and np.float16(exact) == np.float16(3 + 2.0 ** -9)
    rows = np.zeros((2, 32), np.uint8)
    rows[:, :16] = 3
    rows[:, 16:20] = qr.header_bytes([1, 1], [0, 0])
    A = et.QuantizedEmbedding(dev(rows), 16, 8, weighted=True)
    X = windex(np.array([2], np.int64), np.array([1, 2], np.int64), np.array([w], np.float32))
    dst = torch.zeros((1, k + 16), dtype=torch.float16, device=DEV)
    et.maplookup_(et.PreallocationStrategy(k), dst, [A], [X])
    assert dst[0, k:].cpu().tolist() == [3.0] * 16


def test_mixed_plan_and_graph_replays():
    """A plain-index INT8 table, a weighted INT4 table, a mean E4M3 table and a weighted MXFP4
    table in one plan behind three prepended rows: the concatenation of the single lookups,
    eager and replayed from a graph after refilling indices and weights in place."""
    As = [tq.table(8, 128, False)[0], table("int", 4, 32, None, False)[0],
          table("e4m3", 8, 48, None, True)[0], table("mxfp4", 4, 128, None, False)[0]]
    v, cp, w = bags()
    Is = [dev(np.random.default_rng(1).integers(2, R + 1, (B, 20)).astype(np.int64)),
          windex(v, cp, w), windex(v, cp, mode="mean"), windex(v, cp, w)]
    k, D = 3, 128 + 32 + 48 + 128
    dst = torch.full((B, k + D + 2), -3.0, device=DEV)
    plan = et.PreallocationPlan(et.PreallocationStrategy(k), dst, As, Is)

    def check():
        want = torch.cat([et.lookup(A, I) for A, I in zip(As, Is)], dim=1)
        assert raw(dst[:, k:k + D]) == raw(want)
        assert (dst[:, :k] == -3).all() and (dst[:, k + D:] == -3).all()

    plan()
    check()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        plan()
    v2, _, w2 = bags(1)
    for X in Is[1:]:
        X.ragged.values.copy_(dev(v2))
        if X.weights is not None:
            X.weights.copy_(dev(w2))
    Is[0].copy_(torch.flip(Is[0], (0,)))
    for _ in range(3):
        dst.fill_(-3.0)
        g.replay()
        check()
    assert et.check_errors() > 0  # the planted indices were counted, nothing faulted
