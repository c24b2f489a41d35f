"""The split sparse SGD over ragged and weighted gradients, the parts that need no GPU: the
exported symbols, the argument and flag rules of et_ragged_sgd_split (status codes before any
device work), the workspace size, the keyword rules of ``update_(..., split=True)``, and a
check in numpy that the GPU tests' own inputs tell the chunked sum from the serial one."""
import ctypes
import os
import re

import numpy as np
import pytest

import ragged_split_ref as rs

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 1 << 20  # dummy device addresses: every call below stops at the host checks


def _desc(L, **kw):
    """A weighted ragged table: 64 entries, 8 bags, weights at 6 * P."""
    d = dict(table=P, ld_table=16, nrows=100, dim=16, reserved=0, delta=2 * P, ld_delta=16,
             idx=3 * P, nnz=64, colptr=4 * P, batch=8, cols_per_page=0, weights=6 * P,
             dweights=0)
    d.update(kw)
    arr = (L.WeightedUpdateDesc * 1)()
    arr[0] = L.WeightedUpdateDesc(*[d[f[0]] for f in L.WeightedUpdateDesc._fields_])
    return arr


def _ragged(L, **kw):
    return _desc(L, **dict(dict(weights=0), **kw))


def _as_adagrad(L, arr, n):
    out = (L.WeightedAdaGradDesc * n)()
    for t in range(n):
        d = arr[t]
        out[t] = L.WeightedAdaGradDesc(d.table, d.ld_table, d.nrows, d.dim, 1, d.delta,
                                       d.ld_delta, d.idx, 1, d.batch, d.cols_per_page, d.colptr,
                                       d.nnz, 5 * P, d.dim, d.weights)
    return out


def test_symbols_exported_and_abi_version():
    from embtab import _lib

    L = _lib.load()
    for name in ("et_ragged_sgd_split_workspace_size", "et_ragged_sgd_split"):
        assert name in _lib.EXPORTS and hasattr(L, name)
    assert L.et_abi_version() == 9
    hdr = open(os.path.join(REPO, "include", "embtab.h")).read()
    assert re.search(r"#define\s+ET_ABI_VERSION\s+9\b", hdr)
    assert "et_ragged_sgd_split(int dtype, const et_weighted_update_desc* descs" in hdr


def test_julia_shim_binds_the_split_update():
    from test_julia_abi import shim_ccalls

    bound = {c[0] for c in shim_ccalls()}
    assert {"et_ragged_sgd_split_workspace_size", "et_ragged_sgd_split"} <= bound
    src = open(os.path.join(REPO, "embeddingtables.jl_amd", "julia",
                            "EmbeddingTablesHIP.jl")).read()
    assert len(re.findall(r"split::Bool = false", src)) == 2


def test_argument_and_flag_rules_need_no_gpu():
    from embtab import _lib

    L = _lib.load()
    f = L.et_ragged_sgd_split
    a = ctypes.addressof

    def call(arr, dtype=_lib.ET_F32, flags=0, n=1):
        return f(dtype, a(arr) if arr is not None else None, n, 0.1, flags, None, 0, None)

    # weights aligned to C: 4 bytes, 8 for Float64 tables
    for dtype, bad, good in ((_lib.ET_F32, 6 * P + 2, 6 * P + 4), (_lib.ET_F16, 6 * P + 1, 6 * P + 4),
                             (_lib.ET_BF16, 6 * P + 3, 6 * P + 4), (_lib.ET_F64, 6 * P + 4, 6 * P + 8)):
        assert call(_desc(_lib, weights=bad), dtype) == -1 and b"aligned" in L.et_last_error()
        assert call(_desc(_lib, weights=good), dtype) == -3
    for make in (_desc, _ragged):
        for dtype in (_lib.ET_I32, _lib.ET_I64, 99):
            assert call(make(_lib), dtype) == -4
        # the opposite of exact
        assert call(make(_lib), flags=_lib.ET_FLAG_EXACT_UPDATE) == -1
        assert b"exact" in L.et_last_error()
        for flag in (_lib.ET_FLAG_SGD_INDEX_ONLY, _lib.ET_FLAG_SGD_APPLY_ONLY,
                     _lib.ET_FLAG_SGD_HOT_PASS, _lib.ET_FLAG_ADAGRAD_ROWWISE):
            assert call(make(_lib), flags=flag) == -4, flag
            assert call(make(_lib), flags=flag | _lib.ET_FLAG_NONTEMPORAL) == -4, flag
        # accepted: they reach the workspace check
        for flag in (0, _lib.ET_FLAG_NONTEMPORAL, _lib.ET_FLAG_EXACT_IF_FAST,
                     _lib.ET_FLAG_F16_FP32_ACC, _lib.ET_FLAG_SGD_UNFUSED,
                     _lib.ET_FLAG_SGD_UNFUSED | _lib.ET_FLAG_SGD_F64_ALPHA):
            for dtype in (_lib.ET_F32, _lib.ET_F64, _lib.ET_F16, _lib.ET_BF16):
                assert call(make(_lib), dtype, flag) == -3, (flag, dtype)
                assert b"workspace" in L.et_last_error()
        # every descriptor check of et_weighted_sgd
        for neg in ("dim", "nrows", "batch", "cols_per_page", "nnz"):
            assert call(make(_lib, **{neg: -1})) == -1, neg
        assert call(make(_lib), n=-1) == -1
        for null in ("table", "delta", "idx", "colptr"):
            assert call(make(_lib, **{null: 0})) == -1, null
        assert call(make(_lib, ld_table=8)) == -1
        assert call(make(_lib, ld_delta=8)) == -1
        assert call(make(_lib, batch=1 << 32)) == -1
        assert call(make(_lib, nnz=1 << 31)) == -1
        assert call(make(_lib, nrows=1 << 32)) == -1
        # no work: nothing to check, nothing to do
        assert call(make(_lib, batch=0)) == 0
        assert call(make(_lib, dim=0)) == 0
        assert call(make(_lib, nnz=0, table=0, delta=0, idx=0, colptr=0)) == 0
        # dweights is ignored
        assert call(make(_lib, dweights=7 * P + 1)) == -3
    assert call(None, n=0) == 0
    assert call(None, n=1) == -1
    big = (_lib.WeightedUpdateDesc * 33)()
    assert call(big, n=33) == -1 and b"32" in L.et_last_error()
    # a weighted and an unweighted table in one call stop at the workspace, not before
    two = (_lib.WeightedUpdateDesc * 2)(_ragged(_lib)[0], _desc(_lib)[0])
    assert call(two, n=2) == -3


def test_workspace_size_is_the_weighted_adagrad_one_and_the_calls_own_check():
    from embtab import _lib

    L = _lib.load()
    f = L.et_ragged_sgd_split_workspace_size
    nb, na = ctypes.c_int64(-1), ctypes.c_int64(-1)
    assert f(ctypes.addressof(_desc(_lib)), 1, None) == -1
    assert f(None, 1, ctypes.byref(nb)) == -1
    assert f(ctypes.addressof(_desc(_lib, nnz=-1)), 1, ctypes.byref(nb)) == -1
    assert f(ctypes.addressof(_desc(_lib, nnz=1 << 31)), 1, ctypes.byref(nb)) == -1
    big = (_lib.WeightedUpdateDesc * 33)()
    assert f(ctypes.addressof(big), 33, ctypes.byref(nb)) == -1
    sizes = []
    for make in (_desc, _ragged):
        for nnz in (0, 32, 4000, 400000, 10000000):
            for dim in (1, 16, 200, 2048, 3000):
                d = make(_lib, nnz=nnz, dim=dim, ld_table=dim, ld_delta=dim)
                assert f(ctypes.addressof(d), 1, ctypes.byref(nb)) == 0
                ad = _as_adagrad(_lib, d, 1)
                assert L.et_weighted_adagrad_workspace_size(ctypes.addressof(ad), 1,
                                                            ctypes.byref(na)) == 0
                assert nb.value == na.value > 0, (nnz, dim)
                sizes.append(nb.value)
    assert len(set(sizes)) > 10
    # three tables, one of them without work
    three = (_lib.WeightedUpdateDesc * 3)(_ragged(_lib, nnz=5000)[0], _desc(_lib, dim=40, ld_table=40,
                                                                          ld_delta=40)[0],
                                          _desc(_lib, dim=512, ld_table=512, ld_delta=512,
                                                batch=0)[0])
    assert f(ctypes.addressof(three), 3, ctypes.byref(nb)) == 0
    ad = _as_adagrad(_lib, three, 3)
    assert L.et_weighted_adagrad_workspace_size(ctypes.addressof(ad), 3, ctypes.byref(na)) == 0
    assert nb.value == na.value
    # the call's own check is the same carve: one byte short names the number it told
    d = _desc(_lib, nnz=3000)
    assert f(ctypes.addressof(d), 1, ctypes.byref(nb)) == 0
    for base, pad in ((1 << 24, 0), ((1 << 24) + 1, 255)):
        need = nb.value - 256 + pad
        rc = L.et_ragged_sgd_split(_lib.ET_F32, ctypes.addressof(d), 1, 0.1, 0,
                                   ctypes.c_void_p(base), need - 1, None)
        assert rc == -3 and re.search(rb"\b%d bytes" % need, L.et_last_error())


def test_python_keyword_rules():
    import torch

    import embtab as et

    A = et.SimpleEmbedding(torch.zeros((10, 16)))
    gw = et.SparseEmbeddingUpdate(A.lookup_type, torch.zeros((4, 16)),
                                  torch.ones((4, 2), dtype=torch.int64), torch.ones(8))
    gr = et.SparseEmbeddingUpdate(
        A.lookup_type, torch.zeros((4, 16)),
        et.RaggedIndices(torch.ones(8, dtype=torch.int64),
                         torch.tensor([1, 3, 5, 7, 9], dtype=torch.int64)))
    opt = et.Descent(0.1)
    for args in ((A, gw), ([A], [gw]), (A, gr), ([A], [gr])):
        with pytest.raises(et.ArgumentError, match="exact=True"):
            et.update_(opt, *args, split=True, exact=True)
        with pytest.raises(et.ArgumentError, match="hot_pass"):
            et.update_(opt, *args, split=True, hot_pass=True)
        with pytest.raises(et.ArgumentError, match="split"):
            et.update_(et.AdaGrad(weighted=True), *args, split=True)
    # exact=False and exact=None are fine: on the CPU the call gets as far as the device check
    for args in ((A, gw), ([A], [gw])):
        for exact in (False, None):
            with pytest.raises(et.ArgumentError, match="device memory"):
                et.update_(opt, *args, split=True, exact=exact)
        # split=False, the default: a weighted gradient with exact=False still raises
        with pytest.raises(et.ArgumentError, match="exact=False"):
            et.update_(opt, *args, exact=False)
        with pytest.raises(et.ArgumentError, match="exact=False"):
            et.update_(opt, *args, exact=False, split=False)
    with pytest.raises(et.ArgumentError, match="Descent"):
        et.update_(A, gr, et.Indexer(), 0.1, split=True)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("name", ["f32", "f64"])
def test_gpu_inputs_tell_the_chunked_sum_from_the_serial_one(name, weighted):
    """On the GPU tests' own inputs the split model differs from the serial model in the hot
    column and equals it on every column of at most ET_SGD_CHUNK entries, so the GPU
    comparison can tell the two paths apart."""
    kind = rs.KINDS[name]
    dim = 8
    L, values, colptr = rs.split_case(1)
    rng = np.random.default_rng(5)
    delta = kind.fromf(rng.standard_normal((len(L), dim)))
    w = rs.case_weights(1, values, colptr, kind.C) if weighted else None
    ent, g_split = rs.gradient_sums(kind, delta, values, colptr, w)
    _, g_serial = rs.gradient_sums(kind, delta, values, colptr, w, serial=True)
    assert set(g_split) == set(g_serial)
    hot = rs.HOT - 1
    assert len(ent[hot]) == 3000 + rs.HEAD and -(-len(ent[hot]) // rs.CHUNK) == 12
    assert len(ent[hot]) - 11 * rs.CHUNK == 187
    assert [b for b, _ in ent[hot][:rs.HEAD]] == [0] * rs.HEAD  # the uncovered head shifts it
    assert (g_split[hot] != g_serial[hot]).any()
    short = [c for c in g_split if len(ent[c]) <= rs.CHUNK]
    assert len(short) >= 40 and {r - 1 for r, n in rs.FORCED.items() if n <= rs.CHUNK} <= set(short)
    for c in short:
        assert g_split[c].tobytes() == g_serial[c].tobytes(), c
    assert {len(ent[r - 1]) for r in rs.FORCED} == {255, 256, 257, 512, 513}
    assert rs.LONELY - 1 in ent and rs.LONELY - 1 not in g_split  # uncovered entries only
    # and the updated tables differ exactly where the sums do
    table = kind.fromf(rng.standard_normal((rs.ROWS, dim)))
    a = rs.apply(kind, table.copy(), g_split, fused=name == "f32")
    b = rs.apply(kind, table.copy(), g_serial, fused=name == "f32")
    assert (a[hot] != b[hot]).any()
    assert a[[c for c in short]].tobytes() == b[[c for c in short]].tobytes()
    untouched = np.setdiff1d(np.arange(rs.ROWS), sorted(g_split))
    assert len(untouched) > 500 and a[untouched].tobytes() == table[untouched].tobytes()
