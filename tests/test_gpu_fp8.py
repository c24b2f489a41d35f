"""FP8 rows on the GPU (et_fp8_quantize_rows, et_fp8_maplookup_prealloc,
et.QuantizedEmbedding(format=...)) against the numpy restatement (tests/fp8_ref.py).  Every
comparison is byte equality.  Shapes: R = 300 rows; dims 16 / 48 / 128 (1, 3 masked and 8 lanes
per bag of the vector kernel) and 20 (generic); pools 1, 2 and 33 (past the 8 rows in flight,
no multiple of 4); batches 7 and 1027."""
import numpy as np
import pytest
import torch

import fp8_ref as fr
import quant_ref as qr
import test_gpu_quant as tq
from test_gpu_ragged import colptr_of, mix_lengths, ranges_of

pytestmark = pytest.mark.gpu

et = pytest.importorskip("embtab")
from embtab import _lib  # noqa: E402

DEV, R, dev, raw = tq.DEV, tq.R, tq.dev, tq.raw
FMTS = ("e4m3", "e5m2")
DIMS = (16, 48, 128, 20)
_TABLES = {}


def place(rows, hdr, dim, fmt, offset=0):
    """The packed rows on the device, `offset` bytes past a 16-byte boundary."""
    n, ld = rows.shape
    buf = torch.full((n * ld + 32,), 0x5A, dtype=torch.uint8, device=DEV)
    base = (-buf.data_ptr()) % 16 + offset
    packed = buf[base:base + n * ld].view(n, ld)
    packed.copy_(dev(rows))
    return et.QuantizedEmbedding(packed, dim, 8, None if hdr is None else dev(hdr), format=fmt)


def table(fmt, dim, split, offset=0):
    """(table on the device with 0xA5 padding, its dequantised Float32 reference), built once."""
    key = (fmt, dim, split, offset)
    if key not in _TABLES:
        c, s, b = fr.quantize(tq.source_rows(dim, 100 + dim), fmt)
        ld = et.quant.default_ld_bytes(dim, 8, split) + (16 if dim == 48 else 0)
        rows, hdr = fr.rows_of(c, s, b, ld, split, fill=0xA5)
        _TABLES[key] = (place(rows, hdr, dim, fmt, offset), fr.dequantize(c, s, b, fmt))
    return _TABLES[key]


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("dim", (16, 20))
def test_decode_every_code(fmt, dim):
    """Every finite code, with scale 1 and bias 0 and with a scale and bias per row."""
    codes = fr.finite_codes(fmt)
    assert len(codes) == (254 if fmt == "e4m3" else 248)
    n = -(-len(codes) // dim)
    c = np.zeros(n * dim, np.uint8)
    c[:len(codes)] = codes
    c = c.reshape(n, dim)
    rng = np.random.default_rng(3)
    for s, b in ((np.ones(n), np.zeros(n)), (rng.uniform(1e-3, 40, n), rng.normal(0, 50, n))):
        s, b = s.astype(np.float16), b.astype(np.float16)
        Q = place(*fr.rows_of(c, s, b, et.quant.default_ld_bytes(dim, 8), False), dim, fmt)
        got = et.lookup(Q, torch.arange(1, n + 1, device=DEV))
        assert raw(got) == fr.dequantize(c, s, b, fmt).tobytes()
    assert et.check_errors() == 0


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("dim", DIMS)
def test_quantiser_matches_the_reference(fmt, dim):
    L = _lib.load()
    x = tq.source_rows(dim, 7 * dim)
    xd = dev(x)
    c, s, b = fr.quantize(x, fmt)
    assert np.isfinite(fr.decode_table(fmt)[c]).all() and (s[[0, 1]] == 1).all()
    for split in (False, True):
        for ld in (tq.min_ld(dim, 8, split), tq.min_ld(dim, 8, split) + 12):
            want_rows, want_hdr = fr.rows_of(c, s, b, ld, split, fill=0xA5)
            rows = torch.full((R, ld), 0xA5, dtype=torch.uint8, device=DEV)
            hdr = torch.full((R + 1, 4), 0xA5, dtype=torch.uint8, device=DEV) if split else None
            _lib.check(L.et_fp8_quantize_rows(et.quant.FORMATS[fmt][0], xd.data_ptr(), dim, R, dim,
                                              rows.data_ptr(), ld, hdr.data_ptr() if split else None,
                                              _lib.stream_handle(DEV)))
            assert raw(rows) == want_rows.tobytes(), (split, ld)
            if split:
                assert raw(hdr[:R]) == want_hdr.tobytes() and (hdr[R] == 0xA5).all()
    Q = et.QuantizedEmbedding.quantize(xd, format=fmt)
    assert Q.format == fmt and Q.ld_bytes == et.quant.default_ld_bytes(dim, 8)
    assert raw(Q.packed) == fr.rows_of(c, s, b, Q.ld_bytes, False)[0].tobytes()
    assert raw(Q.dequantize()) == fr.dequantize(c, s, b, fmt).tobytes()


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("dim,offset", [(d, 0) for d in DIMS] + [(128, 4)])
def test_pooled_lookup(fmt, dim, offset):
    """Strided destinations of every type, ragged bags, the float kernels on dequantize();
    offset 4 puts vector-shaped rows on the generic kernel."""
    rng = np.random.default_rng(11)
    for split in (False, True):
        Q, T = table(fmt, dim, split, offset)
        S = et.SimpleEmbedding(Q.dequantize())
        assert raw(S.data) == T.tobytes()
        for P, B in ((1, 7), (2, 1027), (33, 7), (33, 1027)):
            idx = tq.indices(B, P, 1000 * P + B)
            I = dev(idx[:, 0] if P == 1 else idx)
            for name, dt in tq.OUTS:
                wide = torch.full((B, dim + 5), -3.0, dtype=dt, device=DEV)
                et.lookup_(wide[:, 3:3 + dim], Q, I)
                want = qr.store(np.full((B, dim + 5), -3.0, np.float32), name)
                want[:, 3:3 + dim] = qr.pooled_matrix(T, idx, name)
                assert raw(wide) == want.tobytes(), (split, P, B, name)
            assert raw(et.lookup(Q, I)) == raw(et.lookup(S, I))
        L = mix_lengths(40, rng)
        v, cp = rng.integers(1, R + 1, int(L.sum())).astype(np.int64), colptr_of(L)
        rag = et.RaggedIndices(dev(v), dev(cp))
        want, _ = qr.pooled(T, [v[lo:hi] for lo, hi in ranges_of(cp, len(v))])
        assert raw(et.lookup(Q, rag)) == want.tobytes() == raw(et.lookup(S, rag))
    assert et.check_errors() == 0


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("dim", (128, 48, 20))
def test_out_of_range_indices_add_zero(fmt, dim):
    """Row 1 holds NaN codes (E5M2: and Inf codes): an out-of-range index must not read them."""
    c, s, b = fr.quantize(tq.source_rows(dim, 5), fmt)
    c[0] = 0x7F
    if fmt == "e5m2":
        c[0, dim // 2:] = 0xFC
    T = fr.dequantize(c, s, b, fmt)
    assert not np.isfinite(T[0]).any()
    Q = place(*fr.rows_of(c, s, b, et.quant.default_ld_bytes(dim, 8), False), dim, fmt)
    et.check_errors()
    for B, P in ((7, 20), (67, 33)):
        idx = np.maximum(tq.indices(B, P, 5 * B + P), 2)
        idx[0, 0], idx[B // 2, P // 2], idx[-1, -1], idx[1, 8], idx[1, 9] = 0, R + 1, -5, R + 1, 0
        want, oob = qr.pooled(T, idx)
        assert oob == 5 and np.isfinite(want).all()
        assert raw(et.lookup(Q, dev(idx))) == want.tobytes(), (B, P)
        assert et.check_errors() == oob


@pytest.mark.parametrize("fmt", FMTS)
def test_mixed_list_and_graph_replay(fmt):
    """INT8, this format (ragged), the other format (split) and INT4 in one plan behind three
    prepended rows, eager and replayed from a graph on new indices."""
    other = FMTS[1 - FMTS.index(fmt)]
    tabs = [tq.table(8, 128, False), table(fmt, 48, False), table(other, 20, True),
            tq.table(4, 32, False)]
    Qs, Ts = [q for q, _ in tabs], [t for _, t in tabs]
    rng = np.random.default_rng(51)
    B, k = 67, 3
    L = mix_lengths(B, rng)
    cp = colptr_of(L)
    i0, i2, i3 = (dev(tq.indices(B, P, 60 + P)) for P in (20, 5, 2))
    v = dev(rng.integers(1, R + 1, int(L.sum())).astype(np.int64))
    dst = torch.full((B, k + 228 + 2), -3.0, device=DEV)
    plan = et.PreallocationPlan(et.PreallocationStrategy(k), dst,
                                Qs, [i0, et.RaggedIndices(v, dev(cp)), i2, i3])

    def expect():
        want = np.full((B, k + 230), -3.0, np.float32)
        vh = v.cpu().numpy()
        want[:, k:k + 228] = np.concatenate(
            [qr.pooled_matrix(Ts[0], i0.cpu().numpy()),
             qr.pooled(Ts[1], [vh[lo:hi] for lo, hi in ranges_of(cp, len(vh))])[0],
             qr.pooled_matrix(Ts[2], i2.cpu().numpy()),
             qr.pooled_matrix(Ts[3], i3.cpu().numpy())], axis=1)
        return want.tobytes()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        plan()
    torch.cuda.current_stream().wait_stream(side)
    assert raw(dst) == expect()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        plan()
    for seed in (83, 85):
        i0.copy_(dev(tq.indices(B, 20, seed)))
        i2.copy_(dev(tq.indices(B, 5, seed)))
        v.copy_(dev(rng.integers(1, R + 1, len(v)).astype(np.int64)))
        dst.fill_(-3.0)
        g.replay()
        assert raw(dst) == expect(), seed
    assert et.check_errors() == 0
