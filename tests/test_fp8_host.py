"""FP8 rows, the parts that need no GPU: the C ABI of et_fp8_quantize_rows and
et_fp8_maplookup_prealloc (symbols, every sampled argument error before any device work) and
the Python class's `format` argument."""
import ctypes

import numpy as np
import pytest
import torch

import fp8_ref as fr
from test_quant_host import P, _desc


def test_symbols_and_lookup_argument_errors_need_no_gpu():
    from embtab import _lib

    L = _lib.load()
    assert hasattr(L, "et_fp8_quantize_rows") and hasattr(L, "et_fp8_maplookup_prealloc")
    assert L.et_abi_version() == 9

    def call(arr, fmt=1, dtype=_lib.ET_F32, flags=0, n=1, batch=8, dst=2 * P, ld_dst=128):
        return L.et_fp8_maplookup_prealloc(dtype, fmt, ctypes.addressof(arr) if arr else None, n,
                                           batch, dst, ld_dst, flags, None)

    for fmt in (0, 3, -1):
        assert call(_desc(_lib), fmt) == -4 and b"format" in L.et_last_error()
    for fmt in (1, 2):
        assert call(_desc(_lib, bits=4, ld_bytes=80), fmt) == -1 and b"bits" in L.et_last_error()
        # the shared rules, sampled: destination type, flags, ld_bytes, sizes, NULLs, bounds
        assert call(_desc(_lib), fmt, dtype=_lib.ET_F64) == -4
        assert call(_desc(_lib), fmt, flags=_lib.ET_FLAG_F16_FP32_ACC) == -4
        assert call(_desc(_lib, ld_bytes=128), fmt) == -1 and b"ld_bytes" in L.et_last_error()
        assert call(_desc(_lib, pool=-1), fmt) == -1
        assert call((_lib.QuantDesc * 33)(), fmt, n=33) == -1
        assert call(None, fmt) == -1
        assert call(_desc(_lib), fmt, ld_dst=127) == -1
        assert call(_desc(_lib), fmt, batch=0) == 0


def test_quantize_argument_errors_need_no_gpu():
    from embtab import _lib

    L = _lib.load()
    ok = dict(fmt=1, src=P, ld_src=128, nrows=10, dim=128, table=2 * P, ld_bytes=144, hdr=None)

    def call(**kw):
        d = {**ok, **kw}
        return L.et_fp8_quantize_rows(d["fmt"], d["src"], d["ld_src"], d["nrows"], d["dim"],
                                      d["table"], d["ld_bytes"], d["hdr"], None)

    assert call(fmt=0) == -4 and call(fmt=3) == -4 and b"format" in L.et_last_error()
    for fmt in (1, 2):
        assert call(fmt=fmt, ld_bytes=128) == -1            # fused: payload + 4
        assert call(fmt=fmt, ld_bytes=124, hdr=3 * P) == -1  # split: payload
        assert call(fmt=fmt, nrows=-1) == -1 and call(fmt=fmt, ld_src=64) == -1
        assert call(fmt=fmt, src=None) == -1 and call(fmt=fmt, table=None) == -1
        assert call(fmt=fmt, nrows=0) == 0


@pytest.mark.parametrize("fmt", ["e4m3", "e5m2"])
def test_python_format_argument(fmt):
    import embtab as et

    x = np.random.default_rng(5).standard_normal((10, 20)).astype(np.float32) - 100
    codes, scale, bias = fr.quantize(x, fmt)
    rows, _ = fr.rows_of(codes, scale, bias, 32, False)
    Q = et.QuantizedEmbedding(torch.from_numpy(rows), 20, 8, format=fmt)
    assert Q.format == fmt and fmt.upper() in repr(Q) and Q.size() == (20, 10)
    assert et.QuantizedEmbedding(torch.from_numpy(rows), 20, 8).format == "int"
    ref = fr.dequantize(codes, scale, bias, fmt)
    assert Q.dequantize().numpy().tobytes() == ref.tobytes()
    for kw in (dict(bits=4, format=fmt), dict(bits=8, format="e3m4"), dict(bits=8, format=None)):
        with pytest.raises(et.ArgumentError):
            et.QuantizedEmbedding(torch.from_numpy(rows), 20, kw["bits"], None, kw["format"])
        with pytest.raises(et.ArgumentError):
            et.QuantizedEmbedding.quantize(torch.zeros((4, 16)), kw["bits"], format=kw["format"])
    # a CPU table is refused as an INT8 one is
    I = torch.ones((4, 2), dtype=torch.int64)
    with pytest.raises(et.ArgumentError, match="device memory"):
        et.lookup(Q, I)
    with pytest.raises(TypeError, match="QuantizedEmbedding"):
        et.rrule(et.lookup, Q, I)
