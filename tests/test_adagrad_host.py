"""Sparse AdaGrad, the parts that need no GPU: the argument and dtype errors of
et_adagrad_workspace_size / et_sparse_adagrad (status codes before any device work), the
workspace size, the ctypes mirror of et_adagrad_desc, and the keywords update_ refuses for
an AdaGrad optimiser."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 1 << 20  # dummy device addresses: every call below stops at the host checks


def _desc(L, **kw):
    d = dict(table=P, ld_table=16, nrows=100, dim=16, pool=4, delta=2 * P, ld_delta=16,
             idx=3 * P, ld_idx=4, batch=8, cols_per_page=0, colptr=0, nnz=0, state=5 * P,
             ld_state=16)
    d.update(kw)
    arr = (L.AdaGradDesc * 1)()
    arr[0] = L.AdaGradDesc(*[d[f[0]] for f in L.AdaGradDesc._fields_])
    return arr


def _ragged(L, **kw):
    d = dict(pool=0, ld_idx=0, colptr=4 * P, nnz=64)
    d.update(kw)
    return _desc(L, **d)


def test_struct_layout_matches_header(tmp_path):
    from embtab import _lib

    S = _lib.AdaGradDesc
    fields = [f[0] for f in S._fields_]
    fmt = " ".join(["%zu"] * (len(fields) + 1))
    args = ", ".join(["sizeof(et_adagrad_desc)"] +
                     [f"offsetof(et_adagrad_desc, {f})" for f in fields])
    prog = tmp_path / "layout.c"
    prog.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "embtab.h"\n'
                    f'int main(void) {{\n  printf("{fmt}\\n", {args});\n'
                    '  printf("%u\\n", ET_FLAG_ADAGRAD_ROWWISE);\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), str(prog), "-o", str(exe)],
                   check=True)
    l1, l2 = subprocess.run([str(exe)], capture_output=True, text=True,
                            check=True).stdout.split("\n")[:2]
    assert list(map(int, l1.split())) == [ctypes.sizeof(S)] + [getattr(S, f).offset
                                                              for f in fields]
    assert int(l2) == _lib.ET_FLAG_ADAGRAD_ROWWISE == 512


def test_julia_shim_binds_adagrad():
    """The shim's AdaGradDesc has the header's fields in order, and both entry points are
    bound (tests/test_julia_abi.py checks every ccall's argument classes against the header)."""
    from test_julia_abi import JL_FIELD, header_structs, shim_ccalls, shim_structs

    jf = [(n, JL_FIELD[t]) for n, t in shim_structs()["AdaGradDesc"]]
    assert jf == header_structs()["et_adagrad_desc"]
    bound = {c[0] for c in shim_ccalls()}
    assert {"et_adagrad_workspace_size", "et_sparse_adagrad"} <= bound


def test_update_argument_errors_need_no_gpu():
    from embtab import _lib

    L = _lib.load()
    f = L.et_sparse_adagrad
    a = ctypes.addressof
    ROW = _lib.ET_FLAG_ADAGRAD_ROWWISE

    def call(arr, dtype=_lib.ET_F32, flags=0, n=1):
        return f(dtype, a(arr) if arr is not None else None, n, 0.1, 1e-8, flags, None, 0, None)

    for make in (_desc, _ragged):
        # element types: the four float types only
        for dtype in (_lib.ET_I32, _lib.ET_I64, 99):
            assert call(make(_lib), dtype) == -4
        # the SGD's flags are refused, each of them
        for flag in (_lib.ET_FLAG_EXACT_UPDATE, _lib.ET_FLAG_EXACT_IF_FAST,
                     _lib.ET_FLAG_SGD_UNFUSED, _lib.ET_FLAG_SGD_F64_ALPHA,
                     _lib.ET_FLAG_SGD_INDEX_ONLY, _lib.ET_FLAG_SGD_APPLY_ONLY,
                     _lib.ET_FLAG_SGD_HOT_PASS):
            assert call(make(_lib), flags=flag) == -4, flag
            assert call(make(_lib), flags=flag | ROW) == -4, flag
        # a NULL state
        assert call(make(_lib, state=0)) == -1 and b"state" in L.et_last_error()
        assert call(make(_lib, state=0), flags=ROW) == -1
        # ld_state < dim: element-wise only (the row-wise form ignores it)
        assert call(make(_lib, ld_state=15)) == -1 and b"ld_state" in L.et_last_error()
        assert call(make(_lib, ld_state=0), flags=ROW) == -3
        # a state that overlaps its table: 100 columns of 16 floats at P
        for st in (P, P + 64, P + 99 * 64 + 60, P - 99 * 64 - 60):
            assert call(make(_lib, state=st)) == -1, st
            assert b"overlaps" in L.et_last_error()
        assert call(make(_lib, state=P + 100 * 64)) == -3   # right behind the table
        assert call(make(_lib, state=P - 100 * 64)) == -3   # right in front of it
        assert call(make(_lib, state=P + 396), flags=ROW) == -1   # 100 floats of state
        assert call(make(_lib, state=P - 400), flags=ROW) == -3
        # negative sizes
        for neg in ("dim", "nrows", "batch", "cols_per_page", "nnz", "pool"):
            assert call(make(_lib, **{neg: -1})) == -1, neg
        assert call(make(_lib), n=-1) == -1
        # other NULLs and leading dimensions
        for null in ("table", "delta", "idx"):
            assert call(make(_lib, **{null: 0})) == -1, null
        assert call(make(_lib, ld_table=8)) == -1
        assert call(make(_lib, ld_delta=8)) == -1
        # valid descriptors stop at the missing workspace, for every type and both forms
        for dtype in (_lib.ET_F32, _lib.ET_F64, _lib.ET_F16, _lib.ET_BF16):
            for flags in (0, ROW, _lib.ET_FLAG_NONTEMPORAL, ROW | _lib.ET_FLAG_NONTEMPORAL):
                assert call(make(_lib), dtype, flags) == -3
                assert b"workspace" in L.et_last_error()
        # nothing to do
        assert call(make(_lib, batch=0)) == 0
        assert call(make(_lib, dim=0)) == 0
    assert call(_desc(_lib, ld_idx=3)) == -1
    assert call(_desc(_lib, pool=0)) == 0
    assert call(_ragged(_lib, nnz=0)) == 0
    assert call(None, n=0) == 0
    assert call(None, n=1) == -1
    big = (_lib.AdaGradDesc * 33)()
    assert call(big, n=33) == -1 and b"32" in L.et_last_error()


def test_workspace_size_errors_and_growth():
    from embtab import _lib

    L = _lib.load()
    f = L.et_adagrad_workspace_size
    nb = ctypes.c_int64(-1)
    assert f(ctypes.addressof(_desc(_lib)), 1, None) == -1
    assert f(None, 1, ctypes.byref(nb)) == -1
    assert f(ctypes.addressof(_desc(_lib, batch=-1)), 1, ctypes.byref(nb)) == -1
    assert f(ctypes.addressof(_ragged(_lib, nnz=-1)), 1, ctypes.byref(nb)) == -1
    big = (_lib.AdaGradDesc * 33)()
    assert f(ctypes.addressof(big), 33, ctypes.byref(nb)) == -1
    assert f(ctypes.addressof(_ragged(_lib, nnz=1 << 31)), 1, ctypes.byref(nb)) == -1
    # monotone in the occurrences, fixed pool (pool * batch) and ragged (nnz) alike
    sizes = []
    for batch in (0, 8, 1000, 100000, 2500000):
        assert f(ctypes.addressof(_desc(_lib, batch=batch)), 1, ctypes.byref(nb)) == 0
        sizes.append(nb.value)
    assert sizes[0] > 0 and sizes == sorted(set(sizes))
    rsizes = []
    for nnz in (0, 32, 4000, 400000, 10000000):
        assert f(ctypes.addressof(_ragged(_lib, nnz=nnz)), 1, ctypes.byref(nb)) == 0
        rsizes.append(nb.value)
    assert rsizes == sorted(set(rsizes))
    # the same occurrences cost the same in either form: 4 x 8 = 32 of them
    assert rsizes[1] == sizes[1]
    # at least the sort's key / value pairs and the bag ids: 5 words per occurrence
    assert rsizes[4] - rsizes[0] >= 10000000 * 20
    # both kinds in one call add up
    two = (_lib.AdaGradDesc * 2)(_desc(_lib, batch=1000)[0], _ragged(_lib, nnz=4000)[0])
    assert f(ctypes.addressof(two), 2, ctypes.byref(nb)) == 0
    assert nb.value > max(sizes[2], rsizes[2])


def test_workspace_one_byte_short():
    """The size told carries 256 bytes of slack for the layout's alignment, as
    et_sgd_workspace_size's does: a workspace that starts `pad` bytes before a 256-byte
    boundary needs size - 256 + pad bytes, one byte less is ET_ERR_WORKSPACE and the message
    names the number (the check comes before any launch)."""
    from embtab import _lib

    L = _lib.load()
    shapes = {
        "fixed": _desc(_lib, batch=128),
        "ragged": _ragged(_lib, nnz=3000),
        "dim 1504": _desc(_lib, dim=1504, ld_table=1504, ld_delta=1504, ld_state=1504,
                          batch=1024, state=1 << 30),
    }
    for name, d in shapes.items():
        nb = ctypes.c_int64(0)
        assert L.et_adagrad_workspace_size(ctypes.addressof(d), 1, ctypes.byref(nb)) == 0
        for base, pad in ((1 << 24, 0), ((1 << 24) + 1, 255), ((1 << 24) + 192, 64)):
            need = nb.value - 256 + pad
            for flags in (0, _lib.ET_FLAG_ADAGRAD_ROWWISE):
                rc = L.et_sparse_adagrad(_lib.ET_F32, ctypes.addressof(d), 1, 0.1, 1e-8, flags,
                                         ctypes.c_void_p(base), need - 1, None)
                assert rc == -3, (name, base, L.et_last_error())
                assert re.search(rb"\b%d bytes" % need, L.et_last_error()), (name, base, need)


def _cpu_case():
    import embtab as et

    A = et.SimpleEmbedding(torch.zeros((10, 16)))
    g = et.SparseEmbeddingUpdate(A.lookup_type, torch.zeros((4, 16)),
                                 torch.ones((4, 2), dtype=torch.int64))
    return et, A, g


@pytest.mark.parametrize("kw", [{"exact": True}, {"exact": False}, {"hot_pass": True},
                                {"f16_fp32_acc": True}, {"indexer": None},
                                {"indexers": [None]}, {"telemetry_cb": lambda: None}])
def test_update_refuses_the_sgd_keywords(kw):
    et, A, g = _cpu_case()
    name = next(iter(kw))
    for args in ((A, g), ([A], [g])):
        with pytest.raises(et.ArgumentError, match=name):
            et.update_(et.AdaGrad(), *args, **kw)
    # a positional indexer is refused too
    with pytest.raises(et.ArgumentError, match="indexer"):
        et.update_(et.AdaGrad(), A, g, et.Indexer())


def test_optimiser_object():
    et, A, g = _cpu_case()
    opt = et.AdaGrad()
    assert (opt.eta, opt.eps, opt.rowwise, opt.initial_accumulator_value) == (0.1, 1e-8, False, 0.0)
    s = opt.state(A)
    assert s.shape == (10, 16) and s.dtype == torch.float32 and not s.any()
    assert opt.state(A) is s                      # kept per table object
    B = et.SimpleEmbedding(torch.zeros((10, 16), dtype=torch.float64))
    assert opt.state(B).dtype == torch.float64 and opt.state(B) is not s
    H = et.SimpleEmbedding(torch.zeros((10, 16), dtype=torch.float16))
    row = et.AdaGrad(eta=0.5, eps=1e-3, rowwise=True, initial_accumulator_value=0.25)
    assert row.state(H).shape == (10,) and row.state(H).dtype == torch.float32
    assert (row.state(H) == 0.25).all()
    wide = torch.zeros((10, 24))
    assert opt.set_state(A, wide[:, 4:20]) is opt.state(A)
    for bad in (torch.zeros((10, 15)), torch.zeros((10, 16), dtype=torch.float64),
                torch.zeros((10, 32))[:, ::2]):
        with pytest.raises(et.ArgumentError):
            opt.set_state(A, bad)
    with pytest.raises(et.ArgumentError):
        et.update_(opt, [A], [g, g])
    # PhasedUpdate stays SGD-only
    with pytest.raises(et.ArgumentError, match="SGD-only"):
        et.PhasedUpdate([], []).update_(opt)
