"""Row-wise quantised tables on the GPU (et_quantize_rows, et_quant_maplookup_prealloc,
et.QuantizedEmbedding) against the numpy restatement of the format (tests/quant_ref.py).
Every comparison is byte equality.

Shapes: R = 300 rows; INT8 dims 16 / 48 / 128 (1, 3 and 8 lanes per bag of the vector kernel:
the exact, the masked and the D = 128 geometry) and 20 (generic); INT4 dims 32 / 96 / 128 and
10 / 2 (generic, headers at odd byte offsets); pools 1, 2, 20 and 33 (past the 8 rows in
flight and not a multiple of them or of 4); batches 1, 7 and 1027 (wave tails with several
bags per wave)."""

import numpy as np
import pytest
import torch

import quant_ref as qr
from test_gpu_ragged import colptr_of, mix_lengths, ranges_of

pytestmark = pytest.mark.gpu

et = pytest.importorskip("embtab")
from embtab import _lib  # noqa: E402

DEV = torch.device("cuda:0")
R = 300
INT8_DIMS, INT4_DIMS = (16, 48, 128, 20), (32, 96, 128, 10, 2)
SHAPES = [(8, d) for d in INT8_DIMS] + [(4, d) for d in INT4_DIMS]
OUTS = (("f32", torch.float32), ("f16", torch.float16), ("bf16", torch.bfloat16))


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def raw(t):
    """A tensor's bytes on the host."""
    return t.contiguous().view(torch.uint8).cpu().numpy().tobytes()


def min_ld(dim, bits, split):
    n = qr.payload_bytes(dim, bits) + (0 if split else 4)
    return max((n + 3) // 4 * 4, 4)


def source_rows(dim, seed):
    """R Float32 rows: a constant row, a zero row, a row spanning +-6e4, a row of magnitude
    1e-6, the rest normal data at several scales and shifts."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((R, dim)) * rng.choice([1e-3, 0.1, 1.0, 30.0], (R, 1)) \
        + rng.choice([0.0, 1.0, -100.0], (R, 1))
    x = x.astype(np.float32)
    x[0] = 3.25
    x[1] = 0.0
    x[2] = rng.standard_normal(dim) * 1e4
    x[2, 0], x[2, -1] = -6e4, 6e4
    x[3] = rng.standard_normal(dim) * 1e-6
    return x


_TABLES = {}


def table(bits, dim, split, offset=0, ld=None):
    """(QuantizedEmbedding on the device with 0xA5 in its padding, the dequantised (R, D)
    Float32 reference table) — built once per shape and never modified."""
    key = (bits, dim, split, offset, ld)
    if key not in _TABLES:
        x = source_rows(dim, 100 + dim + bits)
        ldb = ld or et.quant.default_ld_bytes(dim, bits, split) + (16 if dim == 48 else 0)
        rows, hdr = qr.build_rows(x, bits, ldb, split, fill=0xA5)
        buf = torch.full((R * ldb + 32,), 0x5A, dtype=torch.uint8, device=DEV)
        base = (-buf.data_ptr()) % 16 + offset  # 16-byte aligned, then `offset` bytes off
        packed = buf[base:base + R * ldb].view(R, ldb)
        packed.copy_(dev(rows))
        Q = et.QuantizedEmbedding(packed, dim, bits, dev(hdr) if split else None)
        assert Q.packed.data_ptr() % 16 == offset % 16
        _TABLES[key] = (Q, qr.dequantize(*qr.split_rows(rows, dim, bits, hdr)))
    return _TABLES[key]


def indices(B, P, seed):
    rng = np.random.default_rng(seed)
    idx = rng.integers(1, R + 1, (B, P)).astype(np.int64)
    idx[0, 0], idx[-1, -1] = 1, R
    return idx


# --- 1. the quantiser ----------------------------------------------------------------------------

@pytest.mark.parametrize("bits,dim", SHAPES)
def test_quantiser_matches_the_reference(bits, dim):
    """Packed bytes and headers equal the reference for both header forms, at the minimum
    ld_bytes and with padding, which keeps its 0xA5 fill."""
    L = _lib.load()
    x = source_rows(dim, 7 * dim + bits)
    xd = dev(x)
    for split in (False, True):
        for ld in (min_ld(dim, bits, split), min_ld(dim, bits, split) + 12):
            want_rows, want_hdr = qr.build_rows(x, bits, ld, split, fill=0xA5)
            rows = torch.full((R, ld), 0xA5, dtype=torch.uint8, device=DEV)
            hdr = torch.full((R + 1, 4), 0xA5, dtype=torch.uint8, device=DEV) if split else None
            _lib.check(L.et_quantize_rows(xd.data_ptr(), dim, R, dim, bits, rows.data_ptr(), ld,
                                          hdr.data_ptr() if split else None,
                                          _lib.stream_handle(DEV)))
            assert raw(rows) == want_rows.tobytes(), (split, ld)
            if split:
                assert raw(hdr[:R]) == want_hdr.tobytes() and (hdr[R] == 0xA5).all()
    # the special rows: scale 1 and level 0 for the constant and the zero row; the 1e-6 row's
    # range over 255 levels rounds to a zero half (scale 1), over 15 to a subnormal one
    q, scale, bias = qr.split_rows(want_rows, dim, bits, want_hdr)
    assert (scale[[0, 1]] == 1).all() and not q[[0, 1]].any()
    assert scale[3] == 1 and not q[3].any() if bits == 8 else 0 < scale[3] < 6.1e-5
    assert q[2].max() == 2 ** bits - 1 and q[2].min() == 0
    # the Python constructor: default ld_bytes, zero padding, a strided source
    wide = torch.zeros((R, dim + 3), device=DEV)
    wide[:, 1:1 + dim] = xd
    for split in (False, True):
        Q = et.QuantizedEmbedding.quantize(wide[:, 1:1 + dim], bits=bits, split_header=split)
        ld = et.quant.default_ld_bytes(dim, bits, split)
        w_rows, w_hdr = qr.build_rows(x, bits, ld, split)
        assert Q.ld_bytes == ld and Q.bits == bits and Q.size() == (dim, R)
        assert raw(Q.packed) == w_rows.tobytes()
        assert (Q.header is None) == (not split)
        if split:
            assert raw(Q.header) == w_hdr.tobytes()
        assert raw(Q.dequantize()) == qr.dequantize(*qr.split_rows(w_rows, dim, bits, w_hdr)).tobytes()


# --- 2. fixed-pool lookups -------------------------------------------------------------------------

def check_lookup(Q, T, idx):
    acc = qr.pooled_matrix(T, idx)
    I = dev(idx[:, 0] if idx.shape[1] == 1 else idx)
    for name, dt in OUTS:
        dst = torch.empty((idx.shape[0], T.shape[1]), dtype=dt, device=DEV)
        got = et.lookup_(dst, Q, I)
        assert raw(got) == qr.store(acc, name).tobytes(), (Q, idx.shape, name)
    if idx.shape[1] == 1:  # a one-column matrix is the same sum of one row
        assert raw(et.lookup(Q, dev(idx))) == acc.tobytes()


@pytest.mark.parametrize("bits,dim", SHAPES)
def test_lookup_matches_the_reference(bits, dim):
    for split in (False, True):
        Q, T = table(bits, dim, split)
        for P in (1, 2, 20, 33):
            for B in (1, 7, 1027):
                check_lookup(Q, T, indices(B, P, 1000 * P + B))
    assert et.check_errors() == 0


@pytest.mark.parametrize("bits,dim,ld,offset", [(8, 20, 24, 0), (8, 20, 24, 1), (8, 128, 144, 4),
                                                 (4, 32, 20, 8), (8, 16, 20, 0)])
def test_generic_path_shapes(bits, dim, ld, offset):
    """Rows that are no whole 16-byte vectors (dim 20 at ld_bytes 24), an ld_bytes that is no
    multiple of 16, and vector-shaped rows behind an unaligned table pointer."""
    for split in (False, True):
        Q, T = table(bits, dim, split, offset, ld)
        for P, B in ((1, 7), (2, 1), (20, 1027), (33, 7)):
            check_lookup(Q, T, indices(B, P, 77 * P + B))
    assert et.check_errors() == 0


# --- 3. ragged bags ----------------------------------------------------------------------------------

def expect_ragged(T, values, ranges, out="f32"):
    return qr.pooled(T, [values[lo:hi] for lo, hi in ranges], out)


@pytest.mark.parametrize("bits,dim,split", [(8, 128, False), (4, 32, True), (8, 20, False),
                                            (4, 96, False)])
def test_ragged_lookup(bits, dim, split):
    """Every LENMIX length (0, 1 and a 300-entry bag among them), then the same bags with a
    capacity tail, then a colptr that needs clamping."""
    Q, T = table(bits, dim, split)
    rng = np.random.default_rng(31)
    B = 40
    L = mix_lengths(B, rng)
    values = rng.integers(1, R + 1, int(L.sum())).astype(np.int64)
    colptr = colptr_of(L)
    et.check_errors()
    for tail in (0, 9):
        v = np.concatenate([values, np.full(tail, 10 ** 9, np.int64)])  # never read
        I = et.RaggedIndices(dev(v), dev(colptr))
        assert I.nnz == len(v)
        for name, dt in OUTS:
            want, oob = expect_ragged(T, v, ranges_of(colptr, len(v)), name)
            got = et.lookup_(torch.empty((B, dim), dtype=dt, device=DEV), Q, I)
            assert oob == 0 and raw(got) == want.tobytes(), (tail, name)
    assert et.check_errors() == 0
    # clamping: `values` is a view of a longer buffer of valid indices, so even a kernel that
    # forgot to clamp would read only memory this test owns
    CAP = len(values) - 50
    bad = colptr.copy()
    bad[-1] = len(values) + 400      # claims entries beyond the capacity
    bad[18] = bad[17] - 3            # an interior pair decreases
    buf = dev(np.concatenate([values, values[:600]]))
    I = et.RaggedIndices(buf[:CAP], dev(bad))
    rg = ranges_of(bad, CAP)
    want, _ = expect_ragged(T, values[:CAP], rg)
    assert raw(et.lookup(Q, I)) == want.tobytes()
    clamps = sum((lo != int(bad[j]) - 1) + (hi != int(bad[j + 1]) - 1)
                 for j, (lo, hi) in enumerate(rg))
    assert clamps >= 2 and rg[17][0] == rg[17][1] and rg[-1][1] == CAP
    assert et.check_errors() == clamps


# --- 4. out-of-range indices ---------------------------------------------------------------------------

@pytest.mark.parametrize("bits,dim,split", [(8, 128, False), (4, 128, True), (8, 48, True),
                                            (8, 20, False), (4, 10, False)])
def test_out_of_range_indices_add_zero_rows(bits, dim, split):
    Q, T = table(bits, dim, split)
    et.check_errors()
    for B, P in ((7, 20), (67, 33), (5, 1)):
        idx = indices(B, P, 5 * B + P)
        idx[0, 0], idx[B // 2, P // 2], idx[-1, -1] = 0, R + 1, -5
        if P > 8:
            idx[1, 8], idx[1, 9] = R + 1, 0   # two in one bag, across a batch of rows in flight
        want, oob = qr.pooled(T, idx)
        assert oob == (5 if P > 8 else 3)
        got = et.lookup(Q, dev(idx[:, 0] if P == 1 else idx))
        assert raw(got) == want.tobytes(), (B, P)
        assert et.check_errors() == oob
    # ragged values alike
    vals = indices(1, 30, 9)[0]
    vals[[0, 13, 29]] = (R + 1, 0, -5)
    cp = np.array([1, 1, 12, 31], np.int64)
    want, oob = qr.pooled(T, [vals[0:0], vals[0:11], vals[11:30]])
    assert raw(et.lookup(Q, et.RaggedIndices(dev(vals), dev(cp)))) == want.tobytes()
    assert et.check_errors() == oob == 3


# --- 5. one call, three tables ---------------------------------------------------------------------------

@pytest.mark.parametrize("name,dt", OUTS)
def test_three_tables_one_call(name, dt):
    """INT8 D = 128 fixed pool, INT4 D = 32 ragged, INT8 D = 20 split header; prependrows = 3;
    a destination wider than needed keeps its 0xA5 fill everywhere else."""
    (Q1, T1), (Q2, T2), (Q3, T3) = table(8, 128, False), table(4, 32, False), table(8, 20, True)
    rng = np.random.default_rng(51)
    B, k = 67, 3
    i1 = indices(B, 20, 52)
    L = mix_lengths(B, rng)
    v2 = rng.integers(1, R + 1, int(L.sum()) + 6).astype(np.int64)
    cp = colptr_of(L)
    i3 = indices(B, 5, 53)
    width = k + 128 + 32 + 20 + 5
    dst = torch.full((B, width * dt.itemsize), 0xA5, dtype=torch.uint8, device=DEV).view(dt)
    assert dst.shape == (B, width)
    out = et.maplookup_(et.PreallocationStrategy(k, eltype=dt), dst, [Q1, Q2, Q3],
                        [dev(i1), et.RaggedIndices(dev(v2), dev(cp)), dev(i3)])
    assert out is dst
    want = np.full((B, width), 0xA5A5 if dt.itemsize == 2 else 0xA5A5A5A5,
                   dtype=np.uint16 if dt.itemsize == 2 else np.uint32)
    blocks = [qr.pooled_matrix(T1, i1, name),
              expect_ragged(T2, v2, ranges_of(cp, len(v2)), name)[0],
              qr.pooled_matrix(T3, i3, name)]
    off = k
    for b in blocks:
        want[:, off:off + b.shape[1]] = b.view(want.dtype)
        off += b.shape[1]
    assert raw(dst) == want.tobytes()
    # maplookup allocates the same thing, and the per-table strategies agree
    y = et.maplookup(et.PreallocationStrategy(0, eltype=dt), [Q1, Q3], [dev(i1), dev(i3)])
    assert y.dtype == dt and raw(y) == np.concatenate([blocks[0], blocks[2]], axis=1).tobytes()
    if dt == torch.float32:
        for strat in (et.DefaultStrategy(), et.SimpleParallelStrategy()):
            ys = et.maplookup(strat, [Q1, Q3], [dev(i1), dev(i3)])
            assert [raw(a) for a in ys] == [blocks[0].tobytes(), blocks[2].tobytes()]
    assert et.check_errors() == 0


def test_more_tables_than_one_launch():
    """Lists longer than ET_MAX_TABLES_PER_LAUNCH are split by the binding."""
    Q, T = table(8, 16, False)
    n, B = 35, 7
    idx = [indices(B, 3, 600 + t) for t in range(n)]
    y = et.maplookup(et.PreallocationStrategy(4), [Q] * n, [dev(i) for i in idx])
    want = np.concatenate([qr.pooled_matrix(T, i) for i in idx], axis=1)
    assert y.shape == (B, 4 + 16 * n) and raw(y[:, 4:]) == want.tobytes()


# --- 6. the float path on the dequantised table -------------------------------------------------------------

@pytest.mark.parametrize("bits,dim,split", [(8, 128, False), (4, 128, True), (8, 20, False),
                                            (4, 96, False)])
def test_equals_the_float_lookup_of_the_dequantised_table(bits, dim, split):
    """Ties the new path to the oracle-pinned one: et.lookup on SimpleEmbedding(Q.dequantize())
    and the Float16 store of maplookup_ with eltype=torch.float16."""
    Q, T = table(bits, dim, split)
    S = et.SimpleEmbedding(Q.dequantize())
    assert raw(S.data) == T.tobytes()
    rng = np.random.default_rng(61)
    idx = dev(indices(131, 20, 62))
    L = mix_lengths(40, rng)
    rag = et.RaggedIndices(dev(rng.integers(1, R + 1, int(L.sum())).astype(np.int64)),
                           dev(colptr_of(L)))
    vec = dev(indices(131, 1, 63)[:, 0])
    for I in (idx, rag, vec):
        assert raw(et.lookup(Q, I)) == raw(et.lookup(S, I))
    for I in (idx, vec):
        strat = et.PreallocationStrategy(0, eltype=torch.float16)
        a = et.maplookup(strat, [Q], [I])
        b = et.maplookup(strat, [S], [I])
        assert a.dtype == b.dtype == torch.float16 and raw(a) == raw(b)
    assert et.check_errors() == 0


# --- 7. a quantised and a float call into one destination -----------------------------------------------------

def test_two_calls_fill_one_destination():
    Q, T = table(8, 128, False)
    rng = np.random.default_rng(71)
    F = rng.standard_normal((R, 16)).astype(np.float32)
    S = et.SimpleEmbedding(dev(F))
    B = 67
    iq, ifl = indices(B, 20, 72), indices(B, 4, 73)
    dst = torch.full((B, 2 + 128 + 16), -3.0, device=DEV)
    with pytest.raises(NotImplementedError, match="prependrows"):
        et.maplookup_(et.PreallocationStrategy(2), dst, [Q, S], [dev(iq), dev(ifl)])
    et.maplookup_(et.PreallocationStrategy(2), dst, [Q], [dev(iq)])
    et.maplookup_(et.PreallocationStrategy(2 + 128), dst, [S], [dev(ifl)])
    want = np.full((B, 146), -3.0, np.float32)
    want[:, 2:130] = qr.pooled_matrix(T, iq)
    want[:, 130:] = qr.pooled_matrix(F, ifl)
    assert raw(dst) == want.tobytes()
    assert et.check_errors() == 0


# --- 8. graph capture --------------------------------------------------------------------------------------------

def test_plan_replays_from_a_graph():
    (Q1, T1), (Q2, T2) = table(8, 128, False), table(4, 128, True)
    B, P = 128, 20
    i1, i2 = dev(indices(B, P, 81)), dev(indices(B, P, 82))
    dst = torch.zeros((B, 256), device=DEV)
    plan = et.PreallocationPlan(et.PreallocationStrategy(0), dst, [Q1, Q2], [i1, i2])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        plan()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        plan()
    for seed in (83, 85):
        n1, n2 = indices(B, P, seed), indices(B, P, seed + 1)
        i1.copy_(dev(n1))
        i2.copy_(dev(n2))
        dst.fill_(-1.0)
        g.replay()
        want = np.concatenate([qr.pooled_matrix(T1, n1), qr.pooled_matrix(T2, n2)], axis=1)
        assert raw(dst) == want.tobytes(), seed
    assert et.check_errors() == 0
