"""MXFP4 rows without a GPU: the reference quantiser's derived error bound and pinned blocks,
the argument errors of the two C entries and the Python class's `format="mxfp4"`."""
import ctypes

import numpy as np
import pytest
import torch

import mx4_ref as mr
from test_quant_host import P, _desc


def test_reference_quantiser_error_bound_and_pinned_blocks():
    """|x - v| <= 2^(E+1), E = e - 127.  Derived: e = expfield(amax) - 2 puts amax in
    [4 * 2^E, 8 * 2^E) (below it where e is clamped to 0), so y = x / 2^E has |y| < 8.  Up to 6
    the E2M1 grid's widest gap is 2 and nearest rounding is off by at most 1; a |y| in (6, 8)
    saturates at 6 (OCP's floor rule) and is off by less than 2.  y is exact unless subnormal."""
    rng = np.random.default_rng(7)
    x = rng.standard_normal((64, 96)) * 2.0 ** rng.integers(-140, 120, (64, 3)).repeat(32, axis=1)
    x = x.astype(np.float32)
    x[0, :32] = np.linspace(-7.99, 7.99, 32)         # the saturating band under scale 1
    x[1, :32] = np.float32(2.0 ** -149) * np.arange(32)   # subnormal block: e = 0
    x[2, 32:64] = np.float32(3.0e38) * np.linspace(-1, 1, 32)  # the top binade: e = 252
    codes, e = mr.quantize(x)
    assert e[1, 0] == 0 and e[2, 1] == 252 and (codes < 16).all()
    v = mr.decode(codes, e).astype(np.float64)
    bound = np.repeat(np.ldexp(1.0, e.astype(np.int64) - 127 + 1), 32, axis=1)
    err = np.abs(x.astype(np.float64) - v)
    assert np.isfinite(v).all() and (err <= bound).all()
    px, pcodes, pe = mr.pinned()
    codes, e = mr.quantize(px)
    assert np.array_equal(codes, pcodes) and np.array_equal(e, pe)
    assert np.signbit(mr.decode(pcodes, pe)[2, [5, 12]]).all()  # -0.25 and -0 stay negative zeros
    assert mr.decode(np.full((1, 32), 1, np.uint8), np.array([[0]]))[0, 0] == 2.0 ** -128
    assert np.isinf(mr.decode(np.full((1, 32), 4, np.uint8), np.array([[254]]))).all()
    assert np.isnan(mr.decode(np.zeros((1, 32), np.uint8), np.array([[255]]))).all()


def test_argument_errors_need_no_gpu():
    """Every refusal returns before device work: the pointers are dummies."""
    from embtab import _lib

    L = _lib.load()
    assert L.et_abi_version() == 9
    desc = lambda **kw: _desc(_lib, **{**dict(bits=4, ld_bytes=80), **kw})  # noqa: E731

    def call(arr, dtype=_lib.ET_F32, flags=0, n=1, batch=8, dst=2 * P, ld_dst=128):
        return L.et_mx4_maplookup_prealloc(dtype, ctypes.addressof(arr) if arr else None, n, batch,
                                           dst, ld_dst, flags, None)

    assert call(desc(bits=8, ld_bytes=144)) == -1 and b"bits" in L.et_last_error()
    for dim in (16, 100, 127):
        assert call(desc(dim=dim)) == -1 and b"multiple of 32" in L.et_last_error()
    assert call(desc(ld_bytes=64)) == -1 and b"ld_bytes" in L.et_last_error()  # fused: 64 + 4
    bad = [desc(ld_bytes=60, hdr=5 * P), desc(ld_bytes=70), desc(table=0), desc(idx=0)]
    bad += [desc(**{neg: -1}) for neg in ("dim", "nrows", "pool", "ld_idx", "dst_row_off")]
    assert [call(d) for d in bad] == [-1] * len(bad)
    assert call(desc(), dtype=_lib.ET_F64) == -4 == call(desc(), flags=_lib.ET_FLAG_F16_FP32_ACC)
    assert call(desc(), batch=-1) == -1 and call(desc(), ld_dst=127) == -1
    assert call((_lib.QuantDesc * 33)(), n=33) == -1 and b"32" in L.et_last_error()
    assert call(None) == -1 and call(desc(), dst=None) == -1
    assert call(desc(), batch=0) == 0 and call(desc(ld_bytes=64, hdr=5 * P), batch=0) == 0

    def quant(src=P, ld_src=128, nrows=10, dim=128, table=2 * P, ld_bytes=68, scales=None):
        return L.et_mx4_quantize_rows(src, ld_src, nrows, dim, table, ld_bytes, scales, None)

    assert quant(dim=48) == -1 and b"multiple of 32" in L.et_last_error()
    assert quant(ld_bytes=64) == -1 and quant(ld_bytes=60, scales=3 * P) == -1
    assert quant(ld_bytes=70) == -1 and quant(dim=-32) == -1
    assert quant(nrows=-1) == -1 and quant(ld_src=64) == -1
    assert quant(src=None) == -1 and quant(table=None) == -1
    assert quant(nrows=0) == 0 and quant(nrows=0, ld_bytes=64, scales=3 * P) == 0


@pytest.mark.parametrize("split", [False, True])
def test_python_format_argument(split):
    import embtab as et

    x = np.random.default_rng(5).standard_normal((10, 64)).astype(np.float32) * 100
    codes, e = mr.quantize(x)
    ld = et.quant.default_ld_bytes(64, 4, split, "mxfp4")
    assert ld == (32 if split else 48) and et.quant.default_ld_bytes(128, 4, False, "mxfp4") == 80
    rows, hdr = mr.rows_of(codes, e, ld, split, fill=0xA5)
    hdr = torch.from_numpy(hdr) if split else None
    Q = et.QuantizedEmbedding(torch.from_numpy(rows), 64, 4, hdr, format="mxfp4")
    assert Q.format == "mxfp4" and "MXFP4" in repr(Q) and Q.size() == (64, 10)
    assert Q.dequantize().numpy().tobytes() == mr.decode(codes, e).tobytes()
    z = torch.zeros
    for args in ((torch.from_numpy(rows), 64, 8, hdr),                           # bits
                 (torch.from_numpy(rows), 48, 4, hdr),                           # dim % 32
                 (z((10, 32), dtype=torch.uint8), 64, 4, None),                  # no room: fused
                 (torch.from_numpy(rows), 64, 4, z((10, 2), dtype=torch.uint8)),  # scale width
                 (torch.from_numpy(rows), 64, 4, z((10, 2), dtype=torch.float16))):
        with pytest.raises(et.ArgumentError):
            et.QuantizedEmbedding(*args, format="mxfp4")
    # bits defaults to the format's own; an explicit 8 is refused before anything else
    assert et.quant.check_format("mxfp4", None) == 4 and et.quant.check_format("e4m3", None) == 8
    with pytest.raises(et.ArgumentError, match="bits == 4"):
        et.QuantizedEmbedding.quantize(z((4, 32)), 8, format="mxfp4")
    with pytest.raises(et.ArgumentError, match="device memory"):
        et.QuantizedEmbedding.quantize(z((4, 32)), format="mxfp4")
    # inference only, through the existing refusals
    I = torch.ones((4, 2), dtype=torch.int64)
    g = et.SparseEmbeddingUpdate(Q.lookup_type, z((4, 64)), I)
    with pytest.raises(et.ArgumentError, match="device memory"):
        et.lookup(Q, I)
    for refused in (lambda: et.rrule(et.lookup, Q, I), lambda: et.update_(et.Descent(0.1), Q, g),
                    lambda: et.PhasedUpdate([Q], [g])):
        with pytest.raises(TypeError, match="QuantizedEmbedding"):
            refused()
