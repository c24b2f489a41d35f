"""Row-wise quantised tables, the parts that need no GPU: properties of the numpy reference
(tests/quant_ref.py) that the format's contract rests on, the derived error bound of the
quantiser, the C ABI (symbols, struct layout, every argument error before any device work) and
the Python class's argument errors and inference-only refusals."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import quant_ref as qr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 1 << 20  # dummy device addresses: every call below stops at the host checks


# --- the reference ---------------------------------------------------------------------------

def _random_halves(n, rng):
    """n finite half values over the whole format, subnormal ones included."""
    bits = rng.integers(0, 1 << 16, size=4 * n, dtype=np.uint16)
    h = bits.view(np.float16)
    h = h[np.isfinite(h)][:n - 8]
    sub = np.array([1, 2, 3, 0x3FF, 0x200, 0x8001, 0x83FF, 0x0400], dtype=np.uint16).view(np.float16)
    return np.concatenate([h, sub])


def test_product_is_exact_in_float32():
    """float32(q) * float32(scale) equals the Float64 product for every q and 4,096 random
    half scales: 8 x 11 significant bits fit Float32's 24, so v = q*scale + bias rounds once
    whether or not the expression is contracted."""
    rng = np.random.default_rng(1)
    s = _random_halves(4096, rng)
    assert len(s) == 4096 and (np.abs(s[s != 0]) < 6.2e-5).any()  # subnormal halves present
    q = np.arange(256, dtype=np.float32)[:, None]
    p32 = q * s.astype(np.float32)[None, :]
    p64 = q.astype(np.float64) * s.astype(np.float64)[None, :]
    assert p32.dtype == np.float32
    assert np.array_equal(p32.astype(np.float64), p64)


@pytest.mark.parametrize("bits,dim", [(8, 16), (8, 20), (8, 1), (4, 32), (4, 10), (4, 2)])
def test_pack_unpack_round_trip(bits, dim):
    rng = np.random.default_rng(2)
    q = rng.integers(0, 1 << bits, size=(37, dim)).astype(np.uint8)
    q[0], q[1] = 0, (1 << bits) - 1
    p = qr.pack(q, bits)
    assert p.shape == (37, dim * bits // 8) and p.dtype == np.uint8
    assert np.array_equal(qr.unpack(p, dim, bits), q)
    if bits == 4:  # feature 2k is the low nibble of byte k
        assert np.array_equal(p[:, 0] & 15, q[:, 0]) and np.array_equal(p[:, 0] >> 4, q[:, 1])


@pytest.mark.parametrize("bits", [8, 4])
def test_constant_and_zero_rows(bits):
    x = np.zeros((3, 16), dtype=np.float32)
    x[1] = 3.25
    x[2] = -1e-6
    q, scale, bias = qr.quantize(x, bits)
    assert (scale == np.float16(1.0)).all() and not q.any()
    assert bias[0] == 0 and bias[1] == np.float16(3.25)
    v = qr.dequantize(q, scale, bias)
    assert np.array_equal(v[0], x[0]) and np.array_equal(v[1], x[1])


def _bound_data(rng):
    rows = []
    for scale in (1e-3, 1e-1, 1.0, 30.0, 3000.0):
        for shift in (0.0, 1.0, 100.0):
            rows.append(rng.standard_normal((24, 32)) * scale + shift)
            rows.append(rng.standard_normal((24, 32)) * scale - shift)
    x = np.concatenate(rows).astype(np.float32)
    edge = np.zeros((6, 32), dtype=np.float32)
    edge[0, :2] = (-6e4, 6e4)
    edge[1] = np.linspace(-6e4, -5.9e4, 32)
    edge[2] = rng.standard_normal(32) * 1e-6
    edge[3] = rng.standard_normal(32) * 1e-7 + 1e-4
    edge[4] = 5.0
    edge[5, 3] = 2e-7
    return np.concatenate([x, edge])


@pytest.mark.parametrize("bits", [8, 4])
def test_error_bound(bits):
    """|v - x| <= s/2 + 2^-10 (max(|lo|, |hi|) + (hi - lo)) + L 2^-24 for finite rows with
    |x| <= 6e4.  Derived, not measured: s/2 is the rounding of q; the half roundings of the
    bias and the scale are at most 2^-11 relative each (a bias above lo, or L*s below hi - b,
    clamps by at most that), and twice that also covers the Float32 roundings of x - b, the
    quotient and v (2^-24 relative each); a subnormal scale is off by at most 2^-25, L times
    over at the top level."""
    x = _bound_data(np.random.default_rng(3 + bits))
    assert np.abs(x).max() <= 6e4
    q, scale, bias = qr.quantize(x, bits)
    v = qr.dequantize(q, scale, bias).astype(np.float64)
    L = 2 ** bits - 1
    lo, hi = x.min(axis=1).astype(np.float64), x.max(axis=1).astype(np.float64)
    s = scale.astype(np.float64)
    bound = s / 2 + 2.0 ** -10 * (np.maximum(np.abs(lo), np.abs(hi)) + (hi - lo)) + L * 2.0 ** -24
    err = np.abs(v - x.astype(np.float64)).max(axis=1)
    ratio = (err / bound).max()
    print(f"INT{bits}: largest error / bound = {ratio:.3f}")
    assert (err <= bound).all(), (int(np.argmax(err / bound)), ratio)


def test_ordered_sum_and_stores():
    """The pooled reference: a copy of the first row (-0 survives), in-order Float32 adds, one
    conversion, zero rows for bad indices."""
    t = np.array([[-0.0, 1.0], [1e8, 3.0], [1.0, 2.0 ** -20]], dtype=np.float32)
    y, oob = qr.pooled(t, [[1], [2, 3, 3], [], [0, 3, 4, -5]])
    assert oob == 3 and np.signbit(y[0, 0]) and not y[2].any()
    assert y[1, 0] == np.float32(1e8) and y[3].tolist() == [1.0, 2.0 ** -20]
    assert np.array_equal(qr.pooled_matrix(t, np.array([[2, 3, 3]])), y[1:2])
    assert qr.bf16_rne(np.array([1.0, 1.00390625, 1.01171875], np.float32)).tolist() == \
        [0x3F80, 0x3F80, 0x3F82]


# --- the C ABI ---------------------------------------------------------------------------------

def test_symbols_and_struct_layout(tmp_path):
    from embtab import _lib

    L = _lib.load()
    assert hasattr(L, "et_quantize_rows") and hasattr(L, "et_quant_maplookup_prealloc")
    assert L.et_abi_version() == 9
    S = _lib.QuantDesc
    fields = [f[0] for f in S._fields_]
    fmt = " ".join(["%zu"] * (len(fields) + 1))
    args = ", ".join(["sizeof(et_quant_desc)"] + [f"offsetof(et_quant_desc, {f})" for f in fields])
    prog = tmp_path / "layout.c"
    prog.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "embtab.h"\n'
                    f'int main(void) {{\n  printf("{fmt}\\n", {args});\n  return 0;\n}}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), str(prog), "-o", str(exe)],
                   check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    assert list(map(int, out.split())) == [ctypes.sizeof(S)] + [getattr(S, f).offset
                                                               for f in fields]
    # the header's field list, in order
    from test_julia_abi import header_structs

    assert [n for n, _ in header_structs()["et_quant_desc"]] == fields


def _desc(L, **kw):
    d = dict(table=P, ld_bytes=144, nrows=100, dim=128, bits=8, hdr=0, pool=4, reserved=0,
             idx=3 * P, ld_idx=4, colptr=0, nnz=0, dst_row_off=0)
    d.update(kw)
    arr = (L.QuantDesc * 1)()
    arr[0] = L.QuantDesc(*[d[f[0]] for f in L.QuantDesc._fields_])
    return arr


def test_lookup_argument_errors_need_no_gpu():
    """Every ET_ERR_ARG / ET_ERR_UNSUPPORTED case returns before touching a device (the dummy
    pointers are never dereferenced, and no launch is attempted)."""
    from embtab import _lib

    L = _lib.load()
    f = L.et_quant_maplookup_prealloc
    a = ctypes.addressof

    def call(arr, dtype=_lib.ET_F32, flags=0, n=1, batch=8, dst=2 * P, ld_dst=128):
        return f(dtype, a(arr) if arr is not None else None, n, batch, dst, ld_dst, flags, None)

    # destination types
    for dtype in (_lib.ET_F64, _lib.ET_I32, _lib.ET_I64, 99):
        assert call(_desc(_lib), dtype) == -4
    # flags: ET_FLAG_NONTEMPORAL only
    for flag in (_lib.ET_FLAG_F16_FP32_ACC, _lib.ET_FLAG_EXACT_UPDATE, _lib.ET_FLAG_SGD_UNFUSED,
                 _lib.ET_FLAG_ADAGRAD_ROWWISE, 1 << 20):
        assert call(_desc(_lib), flags=flag) == -4
        assert call(_desc(_lib), flags=flag | _lib.ET_FLAG_NONTEMPORAL) == -4
    # bits
    for bits in (0, 1, 2, 5, 16, -8):
        assert call(_desc(_lib, bits=bits)) == -1 and b"bits" in L.et_last_error()
    # an odd dim with 4 bits
    assert call(_desc(_lib, bits=4, dim=127, ld_bytes=80)) == -1 and b"odd" in L.et_last_error()
    # ld_bytes: too small (fused needs payload + 4, split payload) or not a multiple of 4
    assert call(_desc(_lib, ld_bytes=128)) == -1 and b"ld_bytes" in L.et_last_error()
    assert call(_desc(_lib, ld_bytes=124, hdr=5 * P)) == -1
    assert call(_desc(_lib, ld_bytes=134)) == -1
    assert call(_desc(_lib, bits=4, ld_bytes=64)) == -1
    assert call(_desc(_lib, bits=4, dim=10, ld_bytes=8)) == -1
    assert call(_desc(_lib, ld_bytes=-144)) == -1
    # negative sizes
    for neg in ("dim", "nrows", "pool", "ld_idx", "dst_row_off"):
        assert call(_desc(_lib, **{neg: -1})) == -1, neg
    assert call(_desc(_lib, colptr=4 * P, nnz=-1)) == -1
    assert call(_desc(_lib), n=-1) == -1
    assert call(_desc(_lib), batch=-1) == -1
    # too many tables
    big = (_lib.QuantDesc * 33)()
    assert call(big, n=33) == -1 and b"32" in L.et_last_error()
    # NULLs, rows outside the destination, indices into an empty table
    assert call(None) == -1
    assert call(_desc(_lib), dst=None) == -1
    assert call(_desc(_lib, table=0)) == -1
    assert call(_desc(_lib, idx=0)) == -1
    assert call(_desc(_lib, ld_idx=3)) == -1
    assert call(_desc(_lib, nrows=0)) == -1
    assert call(_desc(_lib, dst_row_off=1)) == -1
    assert call(_desc(_lib), ld_dst=127) == -1
    # nothing to do
    assert call(_desc(_lib), batch=0) == 0
    assert call(None, n=0) == 0
    assert call(_desc(_lib, dim=0, ld_bytes=4)) == 0


def test_quantize_argument_errors_need_no_gpu():
    from embtab import _lib

    L = _lib.load()
    f = L.et_quantize_rows
    ok = dict(src=P, ld_src=128, nrows=10, dim=128, bits=8, table=2 * P, ld_bytes=144, hdr=None)

    def call(**kw):
        d = dict(ok)
        d.update(kw)
        return f(d["src"], d["ld_src"], d["nrows"], d["dim"], d["bits"], d["table"], d["ld_bytes"],
                 d["hdr"], None)

    assert call(bits=3) == -1 and b"bits" in L.et_last_error()
    assert call(bits=4, dim=33, ld_bytes=32) == -1
    assert call(ld_bytes=128) == -1            # fused: payload + 4
    assert call(ld_bytes=124, hdr=3 * P) == -1  # split: payload
    assert call(ld_bytes=146) == -1
    assert call(nrows=-1) == -1
    assert call(dim=-1) == -1
    assert call(ld_src=64) == -1
    assert call(src=None) == -1
    assert call(table=None) == -1
    assert call(nrows=0) == 0


# --- Python --------------------------------------------------------------------------------------

def _cpu_table(bits=8, dim=16, rows=10, split=False):
    import embtab as et

    x = np.random.default_rng(5).standard_normal((rows, dim)).astype(np.float32)
    ld = et.quant.default_ld_bytes(dim, bits, split)
    packed, hdr = qr.build_rows(x, bits, ld, split)
    Q = et.QuantizedEmbedding(torch.from_numpy(packed), dim, bits,
                              torch.from_numpy(hdr) if split else None)
    return et, Q, x


def test_constructor_and_accessors():
    et, Q, x = _cpu_table()
    assert Q.size() == (16, 10) and Q.featuresize == 16 and et.featuresize(Q) == 16
    assert Q.bits == 8 and Q.ld_bytes == 32 and Q.header is None and Q.packed.shape == (10, 32)
    assert Q.dtype == torch.float32
    assert et.quant.default_ld_bytes(128, 8) == 144 and et.quant.default_ld_bytes(128, 4) == 80
    assert et.quant.default_ld_bytes(128, 8, True) == 128
    # dequantize() is the reference's, bit for bit, for both widths and header forms
    for bits, split in ((8, False), (8, True), (4, False), (4, True)):
        _, T, x = _cpu_table(bits, 20 if bits == 8 else 10, 33, split)
        ref = qr.dequantize(*qr.quantize(x, bits))
        assert T.dequantize().numpy().tobytes() == ref.tobytes()
    z = torch.zeros
    for args in ((z((10, 32)), 16, 8),                               # not uint8
                 (z(32, dtype=torch.uint8), 16, 8),                  # not 2-D
                 (z((10, 32), dtype=torch.uint8), 16, 6),            # bits
                 (z((10, 32), dtype=torch.uint8), 15, 4),            # odd dim, 4 bits
                 (z((10, 32), dtype=torch.uint8), 0, 8),             # dim
                 (z((10, 16), dtype=torch.uint8), 16, 8),            # no room for the fused header
                 (z((10, 18), dtype=torch.uint8), 12, 8),            # ld_bytes not a multiple of 4
                 (z((0, 32), dtype=torch.uint8), 16, 8),             # no rows
                 (z((10, 64), dtype=torch.uint8)[:, ::2], 16, 8)):   # strided bytes
        with pytest.raises(et.ArgumentError):
            et.QuantizedEmbedding(*args)
    pk = z((10, 16), dtype=torch.uint8)
    et.QuantizedEmbedding(pk, 16, 8, z((10, 4), dtype=torch.uint8))     # split: payload only
    et.QuantizedEmbedding(pk, 16, 8, z((10, 2), dtype=torch.float16))
    for hdr in (z((9, 4), dtype=torch.uint8), z((10, 2), dtype=torch.uint8),
                z((10, 4), dtype=torch.float32), z((10, 8), dtype=torch.uint8)[:, ::2]):
        with pytest.raises(et.ArgumentError):
            et.QuantizedEmbedding(pk, 16, 8, hdr)
    with pytest.raises(et.ArgumentError):   # quantize() works on device memory only
        et.QuantizedEmbedding.quantize(torch.zeros((4, 16)))
    with pytest.raises(et.ArgumentError):
        et.QuantizedEmbedding.quantize(torch.zeros((4, 16), dtype=torch.float16))


def test_training_and_sharding_refuse_quantised_tables():
    from embtab import sharding

    et, Q, _ = _cpu_table()
    I = torch.ones((4, 2), dtype=torch.int64)
    g = et.SparseEmbeddingUpdate(Q.lookup_type, torch.zeros((4, 16)), I)
    name = "QuantizedEmbedding"
    with pytest.raises(TypeError, match=name):
        et.rrule(et.lookup, Q, I)
    with pytest.raises(TypeError, match=name):
        et.rrule(et.maplookup, et.PreallocationStrategy(0), [Q], [I])
    for opt in (et.Descent(0.1), et.AdaGrad()):
        with pytest.raises(TypeError, match=name):
            et.update_(opt, Q, g)
        with pytest.raises(TypeError, match=name):
            et.update_(opt, [Q], [g])
    with pytest.raises(TypeError, match=name):
        et.update_(Q, g, et.Indexer(), 0.1)
    with pytest.raises(TypeError, match=name):
        et.PhasedUpdate([Q], [g])
    piece = sharding.Piece(0, 0, 8, 0)
    for f in (sharding.piece_table, sharding.compact_piece_table):
        with pytest.raises(TypeError, match=name):
            f(Q, piece)
    with pytest.raises(TypeError, match=name):
        Q.device_table()


def test_mixed_list_names_the_two_call_idiom():
    et, Q, _ = _cpu_table()
    A = et.SimpleEmbedding(torch.zeros((10, 16)))
    I = torch.ones((4, 2), dtype=torch.int64)
    dst = torch.zeros((4, 32))
    for tables in ([Q, A], [A, Q]):
        with pytest.raises(NotImplementedError, match="maplookup_ twice.*prependrows"):
            et.maplookup_(et.PreallocationStrategy(0), dst, tables, [I, I])
        with pytest.raises(NotImplementedError, match="prependrows"):
            et.PreallocationPlan(et.PreallocationStrategy(0), dst, tables, [I, I])
