"""MXFP4 rows on the GPU against the numpy restatement (tests/mx4_ref.py), byte for byte.
R = 300 rows, row 1 NaN (scale byte 255); dims 32 / 96 / 128 / 2048 (1 lane per bag, a masked
group of 4, the D = 128 geometry, the vector kernel's 1024-byte limit) and 96 at ld_bytes 52
(generic); B = 65 bags: more than one workgroup of the D = 128 geometry plus a partial group."""
import numpy as np
import pytest
import torch

import mx4_ref as mr
import quant_ref as qr
import test_gpu_fp8 as tf
import test_gpu_quant as tq

pytestmark = pytest.mark.gpu

et = pytest.importorskip("embtab")

DEV, R, dev, raw = tq.DEV, tq.R, tq.dev, tq.raw
B, _TABLES = 65, {}


def table(dim, split, ld=None):
    """(table on the device with 0xA5 padding, its decoded reference), built once.  Scale bytes
    120..134 keep every sum finite; row 1 has scale byte 255 in every block."""
    key = (dim, split, ld)
    if key not in _TABLES:
        rng = np.random.default_rng(dim + split)
        codes = rng.integers(0, 16, (R, dim)).astype(np.uint8)
        e = rng.integers(120, 135, (R, dim // 32)).astype(np.uint8)
        e[0] = 255
        ldb = ld or et.quant.default_ld_bytes(dim, 4, split, "mxfp4")
        rows, hdr = mr.rows_of(codes, e, ldb, split, fill=0xA5)
        Q = et.QuantizedEmbedding(dev(rows), dim, 4, dev(hdr) if split else None, format="mxfp4")
        _TABLES[key] = (Q, mr.decode(codes, e))
    return _TABLES[key]


def indices(P, seed, bad=False):
    """(B, P) indices into rows 2..R; `bad` plants 0 and R + 1."""
    idx = np.random.default_rng(seed).integers(2, R + 1, (B, P)).astype(np.int64)
    if bad:
        idx[0, 0], idx[B // 2, P // 2], idx[-1, -1] = 0, R + 1, R + 1
    return idx


@pytest.mark.parametrize("ld", (32, 20))
def test_every_code_under_every_scale(ld):
    """Row r has scale byte r - 1 and all 16 codes in both nibble positions (ld_bytes 32: vector
    kernel, 20: generic): nibble order, subnormal results at e = 0, Inf at 254, NaN at 255."""
    k = np.arange(16, dtype=np.uint8)
    codes = np.tile(np.stack([k, 15 - k], axis=1).reshape(-1), (256, 1))
    e = np.arange(256, dtype=np.uint8)[:, None]
    want = mr.decode(codes, e)
    assert want[0, 2] == np.float32(2.0 ** -128) and np.isinf(want[254, 8]) and want[254, 4] > 1e38
    rows = dev(mr.rows_of(codes, e, ld, False, fill=0xA5)[0])
    Q = et.QuantizedEmbedding(rows, 32, 4, format="mxfp4")
    for got in (et.lookup(Q, torch.arange(1, 257, device=DEV)), Q.dequantize()):
        got = got.cpu().numpy()
        assert got[:255].tobytes() == want[:255].tobytes()
        assert np.isnan(got[255]).all()
    assert et.check_errors() == 0


@pytest.mark.parametrize("split", (False, True))
@pytest.mark.parametrize("dim,ld", [(32, None), (96, None), (128, None), (2048, None), (96, 52)])
def test_pooled_sums(dim, ld, split):
    Q, T = table(dim, split, ld)
    S = et.SimpleEmbedding(Q.dequantize()[1:])  # the float kernels on the decoded rows 2..R
    et.check_errors()
    for P in (1, 7, 8, 20):  # every tail of the 8/4/2/1 ladder, and more than one chunk
        idx = indices(P, 10 * dim + P)
        I = dev(idx[:, 0] if P == 1 else idx)
        want = qr.pooled_matrix(T, idx)
        assert raw(et.lookup(Q, I)) == want.tobytes() == raw(et.lookup(S, I - 1)), P
        idx = indices(P, 10 * dim + P, bad=True)  # +0 for a bad index, whatever row 1 holds
        want, oob = qr.pooled(T, idx)
        assert oob == 3 and np.isfinite(want).all()
        assert raw(et.lookup(Q, dev(idx[:, 0] if P == 1 else idx))) == want.tobytes(), P
        assert et.check_errors() == oob
    # ragged bags, a bad index among them
    L = np.resize(np.array([0, 1, 9, 17, 3, 8, 20, 0], np.int64), B)
    v = np.random.default_rng(dim).integers(2, R + 1, int(L.sum())).astype(np.int64)
    v[5] = R + 1
    cp = tf.colptr_of(L)
    want, oob = qr.pooled(T, [v[lo:hi] for lo, hi in tf.ranges_of(cp, len(v))])
    assert raw(et.lookup(Q, et.RaggedIndices(dev(v), dev(cp)))) == want.tobytes()
    assert et.check_errors() == oob == 1
    # 16-bit destinations round once; three prepended rows take the unaligned store path
    idx = indices(20, 3 * dim)
    for name, dt in tq.OUTS:
        dst = torch.full((B, 3 + dim), -3.0, dtype=dt, device=DEV)
        et.maplookup_(et.PreallocationStrategy(3), dst, [Q], [dev(idx)])
        want = qr.store(np.full((B, 3 + dim), -3.0, np.float32), name)
        want[:, 3:] = qr.pooled_matrix(T, idx, name)
        assert raw(dst) == want.tobytes(), name
    assert et.check_errors() == 0


@pytest.mark.parametrize("split", (False, True))
@pytest.mark.parametrize("dim", (32, 96, 128))
def test_quantiser_bytes(dim, split):
    rng = np.random.default_rng(dim)
    x = rng.standard_normal((R, dim)) * 2.0 ** rng.integers(-140, 120, (R, dim // 32)).repeat(32, 1)
    x = x.astype(np.float32)
    x[:4, :32] = mr.pinned()[0]
    x[4, :32] = np.float32(2.0 ** -149) * np.arange(32)  # a subnormal block
    codes, e = mr.quantize(x)
    assert (codes[:4, :32] == mr.pinned()[1]).all() and (e[:4, :1] == mr.pinned()[2]).all()
    Q = et.QuantizedEmbedding.quantize(dev(x), format="mxfp4", split_header=split)
    assert Q.bits == 4 and Q.ld_bytes == et.quant.default_ld_bytes(dim, 4, split, "mxfp4")
    rows, hdr = mr.rows_of(codes, e, Q.ld_bytes, split)  # padding stays zero
    assert raw(Q.packed) == rows.tobytes()
    assert raw(Q.header) == hdr.tobytes() if split else Q.header is None
    assert raw(Q.dequantize()) == mr.decode(codes, e).tobytes()


def test_one_list_five_formats_and_graph_replay():
    """One plan behind three prepended rows against the concatenation of the single lookups,
    eager and replayed from a graph on refilled indices."""
    Qs = [tq.table(8, 128, False)[0], tq.table(4, 32, False)[0], tf.table("e4m3", 48, False)[0],
          tf.table("e5m2", 20, True)[0], table(96, False)[0]]
    Is = [dev(indices(P, 70 + P)) for P in (20, 2, 5, 9)]
    L = np.resize(np.array([0, 1, 9, 17, 3], np.int64), B)
    v = dev(np.random.default_rng(9).integers(2, R + 1, int(L.sum())).astype(np.int64))
    Is.append(et.RaggedIndices(v, dev(tf.colptr_of(L))))
    k, D = 3, 128 + 32 + 48 + 20 + 96
    dst = torch.full((B, k + D + 2), -3.0, device=DEV)
    plan = et.PreallocationPlan(et.PreallocationStrategy(k), dst, Qs, Is)

    def check():
        want = torch.cat([et.lookup(Q, I) for Q, I in zip(Qs, Is)], dim=1)
        assert raw(dst[:, k:k + D]) == raw(want)

    plan()
    check()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        plan()
    for I, P in zip(Is, (20, 2, 5, 9)):
        I.copy_(dev(indices(P, 90 + P)))
    v.copy_(torch.flip(v, (0,)))
    dst.fill_(-3.0)
    g.replay()
    check()
    assert et.check_errors() == 0
