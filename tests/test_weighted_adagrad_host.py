"""Weighted sparse AdaGrad, the parts that need no GPU: the exported symbols, the ctypes mirror
of et_weighted_adagrad_desc, the argument errors of et_weighted_adagrad_workspace_size /
et_weighted_adagrad (status codes before any device work), the workspace size, and the
row-wise bounds of tests/test_gpu_weighted_adagrad.py checked on that file's own inputs with
three summation orders evaluated in C."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import weighted_adagrad_ref as war

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 1 << 20  # dummy device addresses: every call below stops at the host checks


def _desc(L, **kw):
    """A weighted ragged table: 64 entries, 8 bags, weights at 6 * P."""
    d = dict(table=P, ld_table=16, nrows=100, dim=16, pool=0, delta=2 * P, ld_delta=16,
             idx=3 * P, ld_idx=0, batch=8, cols_per_page=0, colptr=4 * P, nnz=64, state=5 * P,
             ld_state=16, weights=6 * P)
    d.update(kw)
    arr = (L.WeightedAdaGradDesc * 1)()
    arr[0] = L.WeightedAdaGradDesc(*[d[f[0]] for f in L.WeightedAdaGradDesc._fields_])
    return arr


def _ragged(L, **kw):
    return _desc(L, **dict(dict(weights=0), **kw))


def _fixed(L, **kw):
    return _desc(L, **dict(dict(pool=4, ld_idx=4, colptr=0, nnz=0, weights=0), **kw))


def test_symbols_exported_and_abi_version():
    from embtab import _lib

    L = _lib.load()
    for name in ("et_weighted_adagrad_workspace_size", "et_weighted_adagrad"):
        assert name in _lib.EXPORTS and hasattr(L, name)
    assert L.et_abi_version() == 9
    hdr = open(os.path.join(REPO, "include", "embtab.h")).read()
    assert re.search(r"#define\s+ET_ABI_VERSION\s+9\b", hdr)


def test_struct_layout_matches_header(tmp_path):
    from embtab import _lib

    S = _lib.WeightedAdaGradDesc
    fields = [f[0] for f in S._fields_]
    assert fields[:-1] == [f[0] for f in _lib.AdaGradDesc._fields_] and fields[-1] == "weights"
    fmt = " ".join(["%zu"] * (len(fields) + 2))
    args = ", ".join(["sizeof(et_weighted_adagrad_desc)", "sizeof(et_adagrad_desc)"] +
                     [f"offsetof(et_weighted_adagrad_desc, {f})" for f in fields])
    prog = tmp_path / "layout.c"
    prog.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "embtab.h"\n'
                    f'int main(void) {{\n  printf("{fmt}\\n", {args});\n  return 0;\n}}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), str(prog), "-o", str(exe)],
                   check=True)
    got = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True,
                                       check=True).stdout.split()))
    assert got == ([ctypes.sizeof(S), ctypes.sizeof(_lib.AdaGradDesc)] +
                   [getattr(S, f).offset for f in fields])
    # the fields of et_adagrad_desc sit where et_adagrad_desc has them
    assert all(getattr(S, f).offset == getattr(_lib.AdaGradDesc, f).offset for f in fields[:-1])


def test_julia_shim_binds_weighted_adagrad():
    from test_julia_abi import JL_FIELD, header_structs, shim_ccalls, shim_structs

    jf = [(n, JL_FIELD[t]) for n, t in shim_structs()["WeightedAdaGradDesc"]]
    assert jf == header_structs()["et_weighted_adagrad_desc"]
    bound = {c[0] for c in shim_ccalls()}
    assert {"et_weighted_adagrad_workspace_size", "et_weighted_adagrad"} <= bound


def test_update_argument_errors_need_no_gpu():
    from embtab import _lib

    L = _lib.load()
    f = L.et_weighted_adagrad
    a = ctypes.addressof
    ROW = _lib.ET_FLAG_ADAGRAD_ROWWISE

    def call(arr, dtype=_lib.ET_F32, flags=0, n=1):
        return f(dtype, a(arr) if arr is not None else None, n, 0.1, 1e-8, flags, None, 0, None)

    # weights need the ragged form
    assert call(_fixed(_lib, weights=6 * P)) == -1 and b"colptr" in L.et_last_error()
    assert call(_fixed(_lib, weights=6 * P), flags=ROW) == -1
    # weights aligned to C: 4 bytes, 8 for Float64 tables
    for dtype, bad, good in ((_lib.ET_F32, 6 * P + 2, 6 * P + 4), (_lib.ET_F16, 6 * P + 1, 6 * P + 4),
                             (_lib.ET_BF16, 6 * P + 3, 6 * P + 4), (_lib.ET_F64, 6 * P + 4, 6 * P + 8)):
        assert call(_desc(_lib, weights=bad), dtype) == -1 and b"aligned" in L.et_last_error()
        assert call(_desc(_lib, weights=good), dtype) == -3
    for make in (_desc, _ragged, _fixed):
        for dtype in (_lib.ET_I32, _lib.ET_I64, 99):
            assert call(make(_lib), dtype) == -4
        for flag in (_lib.ET_FLAG_EXACT_UPDATE, _lib.ET_FLAG_EXACT_IF_FAST,
                     _lib.ET_FLAG_F16_FP32_ACC, _lib.ET_FLAG_SGD_UNFUSED,
                     _lib.ET_FLAG_SGD_F64_ALPHA, _lib.ET_FLAG_SGD_INDEX_ONLY,
                     _lib.ET_FLAG_SGD_APPLY_ONLY, _lib.ET_FLAG_SGD_HOT_PASS):
            assert call(make(_lib), flags=flag) == -4, flag
            assert call(make(_lib), flags=flag | ROW) == -4, flag
        assert call(make(_lib), flags=1 << 30) == -1  # an unknown flag
        assert call(make(_lib, state=0)) == -1 and b"state" in L.et_last_error()
        assert call(make(_lib, state=0), flags=ROW) == -1
        assert call(make(_lib, ld_state=15)) == -1 and b"ld_state" in L.et_last_error()
        assert call(make(_lib, ld_state=0), flags=ROW) == -3
        for st in (P, P + 64, P + 99 * 64 + 60, P - 99 * 64 - 60):
            assert call(make(_lib, state=st)) == -1, st
            assert b"overlaps" in L.et_last_error()
        assert call(make(_lib, state=P + 100 * 64)) == -3
        assert call(make(_lib, state=P + 396), flags=ROW) == -1
        assert call(make(_lib, state=P - 400), flags=ROW) == -3
        for neg in ("dim", "nrows", "batch", "cols_per_page", "nnz", "pool"):
            assert call(make(_lib, **{neg: -1})) == -1, neg
        assert call(make(_lib), n=-1) == -1
        for null in ("table", "delta", "idx"):
            assert call(make(_lib, **{null: 0})) == -1, null
        assert call(make(_lib, ld_table=8)) == -1
        assert call(make(_lib, ld_delta=8)) == -1
        for dtype in (_lib.ET_F32, _lib.ET_F64, _lib.ET_F16, _lib.ET_BF16):
            for flags in (0, ROW, _lib.ET_FLAG_NONTEMPORAL, ROW | _lib.ET_FLAG_NONTEMPORAL):
                assert call(make(_lib), dtype, flags) == -3
                assert b"workspace" in L.et_last_error()
        assert call(make(_lib, batch=0)) == 0
        assert call(make(_lib, dim=0)) == 0
    assert call(_desc(_lib, nnz=0)) == 0
    assert call(_fixed(_lib, ld_idx=3)) == -1
    assert call(None, n=0) == 0
    assert call(None, n=1) == -1
    big = (_lib.WeightedAdaGradDesc * 33)()
    assert call(big, n=33) == -1 and b"32" in L.et_last_error()
    # all three kinds in one call stop at the workspace, not before
    three = (_lib.WeightedAdaGradDesc * 3)(_fixed(_lib)[0], _ragged(_lib)[0], _desc(_lib)[0])
    assert call(three, n=3) == -3


def test_workspace_size_errors_growth_and_the_calls_own_check():
    from embtab import _lib

    L = _lib.load()
    f = L.et_weighted_adagrad_workspace_size
    nb = ctypes.c_int64(-1)
    assert f(ctypes.addressof(_desc(_lib)), 1, None) == -1
    assert f(None, 1, ctypes.byref(nb)) == -1
    assert f(ctypes.addressof(_desc(_lib, nnz=-1)), 1, ctypes.byref(nb)) == -1
    assert f(ctypes.addressof(_fixed(_lib, weights=6 * P)), 1, ctypes.byref(nb)) == -1
    big = (_lib.WeightedAdaGradDesc * 33)()
    assert f(ctypes.addressof(big), 33, ctypes.byref(nb)) == -1
    assert f(ctypes.addressof(_desc(_lib, nnz=1 << 31)), 1, ctypes.byref(nb)) == -1
    sizes = []
    for nnz in (0, 32, 4000, 400000, 10000000):
        assert f(ctypes.addressof(_desc(_lib, nnz=nnz)), 1, ctypes.byref(nb)) == 0
        sizes.append(nb.value)
    assert sizes[0] > 0 and sizes == sorted(set(sizes))  # monotone in nnz
    # the call's own check is the same carve: one byte short names the number it told
    d = _desc(_lib, nnz=3000)
    assert f(ctypes.addressof(d), 1, ctypes.byref(nb)) == 0
    for base, pad in ((1 << 24, 0), ((1 << 24) + 1, 255)):
        need = nb.value - 256 + pad
        for flags in (0, _lib.ET_FLAG_ADAGRAD_ROWWISE):
            rc = L.et_weighted_adagrad(_lib.ET_F32, ctypes.addressof(d), 1, 0.1, 1e-8, flags,
                                       ctypes.c_void_p(base), need - 1, None)
            assert rc == -3 and re.search(rb"\b%d bytes" % need, L.et_last_error())


@pytest.mark.parametrize("name,dim", war.ROW_CASES)
def test_rowwise_bounds_hold_for_cpu_summation_orders(name, dim):
    """The bounds' derivation on the GPU test's own weighted inputs (weights uniform on
    [0.25, 2)), with sequential, reversed and pairwise sums of the squares evaluated in C from
    the bit-exact weighted g.  A ratio of 1 or more would mean the derivation is wrong."""
    import test_gpu_adagrad as ta

    kind = ta.KINDS[name]
    case = war.rowwise_case(name, dim, 0)
    worst = 0.0
    for order in ("sequential", "reversed", "pairwise"):
        t2, s2 = war.rowwise_in_C(kind, case["table"], case["state"], case["g_of"], order)
        rs, rw = war.rowwise_bounds(kind, case["table"], case["state"], case["g_of"], t2, s2)
        print(f"weighted rowwise bound ratio {name} dim {dim} {order}: state {rs:.3f} "
              f"table {rw:.3f}")
        worst = max(worst, rs, rw)
    print(f"weighted rowwise worst ratio {name} dim {dim}: {worst:.3f}")
    assert worst < 1.0


def test_python_binding_takes_weights_with_the_opt_in():
    """An AdaGrad built with weighted=True takes a gradient with weights: on the CPU the call
    gets as far as the device check of the indices.  A default one refuses it as ever, and
    names the opt-in."""
    import torch

    import embtab as et

    A = et.SimpleEmbedding(torch.zeros((10, 16)))
    g = et.SparseEmbeddingUpdate(A.lookup_type, torch.zeros((4, 16)),
                                 torch.ones((4, 2), dtype=torch.int64), torch.ones(8))
    assert et.AdaGrad().weighted is False and et.AdaGrad(weighted=True).weighted is True
    for args in ((A, g), ([A], [g])):
        with pytest.raises(et.ArgumentError, match="device memory"):
            et.update_(et.AdaGrad(weighted=True), *args)
        with pytest.raises(et.ArgumentError, match="weighted=True"):
            et.update_(et.AdaGrad(), *args)
    with pytest.raises(et.ArgumentError, match="SGD-only"):
        et.PhasedUpdate([], []).update_(et.AdaGrad())
