"""et_quant_weighted_maplookup_prealloc without a GPU: every argument error comes back as its
status code before any device work (the dummy pointers are never dereferenced), batch == 0 is a
no-op, the ctypes struct mirrors the header, and the Python opt-in flag."""
import ctypes
import os
import subprocess

import pytest
import torch

et = pytest.importorskip("embtab")
from embtab import _lib  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 1 << 20  # dummy device address, 16-byte aligned
ARG, UNSUPPORTED = -1, -4
NT = _lib.ET_FLAG_NONTEMPORAL


def desc(dim=128, bits=8, ld=144, colptr=P, weights=P, mode=_lib.ET_POOL_SUM):
    return _lib.QuantWeightedDesc(P, ld, 1000, dim, bits, None, P, 4096, colptr, 0, weights, mode, 0)


def call(d, fmt=_lib.ET_QUANT_INT, n=1, batch=64, flags=NT, out=_lib.ET_F32):
    arr = (_lib.QuantWeightedDesc * max(n, 1))(*([d] * max(n, 1)))
    return _lib.load().et_quant_weighted_maplookup_prealloc(out, fmt, ctypes.addressof(arr), n,
                                                            batch, P, 4096, flags, None)


@pytest.mark.parametrize("want,kw", [
    (ARG, dict(d=desc(colptr=None))),
    (ARG, dict(d=desc(mode=2))),
    (UNSUPPORTED, dict(d=desc(mode=_lib.ET_POOL_MEAN))),             # weights with MEAN
    (UNSUPPORTED, dict(d=desc(), flags=NT | _lib.ET_FLAG_F16_FP32_ACC)),
    (UNSUPPORTED, dict(d=desc(), fmt=4)),
    (UNSUPPORTED, dict(d=desc(), out=_lib.ET_F64)),
    (ARG, dict(d=desc(dim=48, bits=4, ld=32), fmt=_lib.ET_QUANT_MXFP4)),  # no whole MX block
    (ARG, dict(d=desc(bits=4), fmt=_lib.ET_FP8_E4M3)),               # an FP8 row has 8 bits
    (ARG, dict(d=desc(ld=128))),                                     # no room for the header
    (ARG, dict(d=desc(weights=P + 2))),
    (ARG, dict(d=desc(), n=_lib.ET_MAX_TABLES_PER_LAUNCH + 1)),
])
def test_argument_errors_come_before_any_device_work(want, kw):
    assert call(**kw) == want, _lib.load().et_last_error()
    assert _lib.load().et_last_error()


def test_empty_batch_is_a_no_op_and_the_symbol_is_exported():
    assert call(desc(), batch=0) == 0 and call(desc(), n=0) == 0
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    assert " T et_quant_weighted_maplookup_prealloc" in out


def test_struct_layout_matches_the_header(tmp_path):
    fields = [n for n, _ in _lib.QuantWeightedDesc._fields_]
    prog = tmp_path / "layout.c"
    prog.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "embtab.h"\n'
                    'int main(void) { printf("%zu", sizeof(et_quant_weighted_desc));\n'
                    + "".join(f'printf(" %zu", offsetof(et_quant_weighted_desc, {n}));\n'
                              for n in fields)
                    + 'printf(" %d %d", ET_QUANT_INT, ET_QUANT_MXFP4); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), str(prog), "-o", str(exe)],
                   check=True)
    got = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True,
                                       check=True).stdout.split()))
    D = _lib.QuantWeightedDesc
    assert got == [ctypes.sizeof(D)] + [getattr(D, n).offset for n in fields] + [
        _lib.ET_QUANT_INT, _lib.ET_QUANT_MXFP4]
    assert got[1:len(fields) + 1] == sorted(got[1:len(fields) + 1])  # the header's field order
    assert [et.quant.FORMATS[k][0] for k in ("int", "e4m3", "e5m2", "mxfp4")] == [
        _lib.ET_QUANT_INT, _lib.ET_FP8_E4M3, _lib.ET_FP8_E5M2, _lib.ET_QUANT_MXFP4]


def test_the_table_opts_in():
    Q = et.QuantizedEmbedding(torch.zeros((8, 20), dtype=torch.uint8), 16, 8)
    I = torch.ones((4, 3), dtype=torch.int64)
    W, M = et.WeightedIndices(I, torch.ones(4, 3)), et.WeightedIndices(I, mode="mean")
    for X in (W, M):
        with pytest.raises(et.ArgumentError, match="weighted=True"):
            X.check_for(Q)
    A = Q.accept_weighted()
    assert A.weighted and not Q.weighted
    assert A.packed.data_ptr() == Q.packed.data_ptr() and A.size() == Q.size()
    assert et.QuantizedEmbedding(Q.packed, 16, 8, weighted=True).weighted
    W.check_for(A)
    M.check_for(A)
    with pytest.raises(et.ArgumentError, match="float32"):
        et.WeightedIndices(I, torch.ones(4, 3, dtype=torch.float64)).check_for(A)
    with pytest.raises(et.ArgumentError, match="quantised"):  # still inference only
        et.weighted.weighted_update_desc(A, torch.zeros(4, 16), W.ragged)
