"""Weighted sparse Adam, the parts that need no GPU: the exported symbols, the ctypes and Julia
mirrors of et_weighted_adam_desc, every argument and flag error of et_weighted_adam (status
codes before any device work), the workspace size, and what ``et.Adam(weighted=True)`` takes."""
import ctypes
import os
import re

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 1 << 20  # dummy device addresses: every call below stops at the host checks
COL = 100 * 16 * 4  # bytes of a 100 x 16 Float32 block
ROW = 512


def _desc(L, **kw):
    """A weighted ragged table: 64 entries, 8 bags, weights at 8 * P."""
    d = dict(table=P, ld_table=16, nrows=100, dim=16, pool=0, delta=2 * P, ld_delta=16,
             idx=3 * P, ld_idx=0, batch=8, cols_per_page=0, colptr=4 * P, nnz=64, m=5 * P,
             ld_m=16, v=6 * P, ld_v=16, step=7 * P, weights=8 * P)
    d.update(kw)
    return L.WeightedAdamDesc(*[d[f[0]] for f in L.WeightedAdamDesc._fields_])


FIXED = dict(pool=4, ld_idx=4, colptr=0, nnz=0, weights=0)


def test_symbols_and_struct_mirrors():
    from embtab import _lib
    from test_julia_abi import JL_FIELD, header_structs, shim_ccalls, shim_structs

    L = _lib.load()
    names = {"et_weighted_adam_workspace_size", "et_weighted_adam"}
    assert names <= set(_lib.EXPORTS) and all(hasattr(L, n) for n in names)
    assert L.et_abi_version() == 9
    S = _lib.WeightedAdamDesc
    fields = [f[0] for f in S._fields_]
    assert fields[:-1] == [f[0] for f in _lib.AdamDesc._fields_] and fields[-1] == "weights"
    assert fields == [n for n, _ in header_structs()["et_weighted_adam_desc"]]
    jf = [(n, JL_FIELD[t]) for n, t in shim_structs()["WeightedAdamDesc"]]
    assert jf == header_structs()["et_weighted_adam_desc"]
    assert names <= {c[0] for c in shim_ccalls()}


OK = (0.9, 0.999)
ARG_ERRORS = [  # (descriptor fields, flags, betas, expected status)
    ({}, 0, OK, -3), ({}, ROW | 1, (0.0, 0.0), -3),  # valid: stops at the missing workspace
    (FIXED, 0, OK, -3), (dict(weights=0), ROW, OK, -3),  # the unweighted kinds
    (dict(FIXED, weights=8 * P), 0, OK, -1),         # weights need the ragged form
    (dict(weights=8 * P + 2), 0, OK, -1),            # weights aligned to C
    (dict(weights=5 * P + COL - 4), 0, OK, -1),      # weights overlap the last element of m
    (dict(weights=5 * P + COL), 0, OK, -3),          # right behind it
    (dict(weights=6 * P - 252), 0, OK, -1),          # 64 weights reach the first element of v
    (dict(weights=6 * P - 256), 0, OK, -3),
    (dict(weights=6 * P + 396), ROW, OK, -1), (dict(weights=6 * P + 400), ROW, OK, -3),
    (dict(weights=7 * P + 4), 0, OK, -1), (dict(weights=P + 64), 0, OK, -1),  # step, the table
    # et_sparse_adam's checks through the new entry
    (dict(m=0), 0, OK, -1), (dict(v=0), 0, OK, -1), (dict(step=0), ROW, OK, -1),
    (dict(ld_m=15), ROW, OK, -1), (dict(ld_v=15), 0, OK, -1), (dict(ld_v=0), ROW, OK, -3),
    (dict(m=P + COL - 4), 0, OK, -1), (dict(v=5 * P + COL - 4), 0, OK, -1),
    (dict(step=5 * P + 8), 0, OK, -1),
    ({}, 0, (1.0, 0.999), -1), ({}, 0, (0.9, -0.1), -1), ({}, 0, (float("nan"), 0.5), -1),
    (dict(dim=-1), 0, OK, -1), (dict(nnz=-1), 0, OK, -1), (dict(table=0), 0, OK, -1),
    (dict(ld_delta=8), 0, OK, -1),
    (dict(batch=0, m=0, v=0, step=0, weights=5 * P), 0, OK, 0),  # no work: nothing is read
    # the SGD's flags, an unknown flag
    ({}, 4, OK, -4), ({}, 256 | ROW, OK, -4), ({}, 8, OK, -4), ({}, 32, OK, -4),
    ({}, 128, OK, -4), ({}, 2, OK, -4), ({}, 1024, OK, -1),
]


@pytest.mark.parametrize("kw,flags,beta,rc", ARG_ERRORS)
def test_argument_errors_need_no_gpu(kw, flags, beta, rc):
    from embtab import _lib

    L = _lib.load()
    arr = (_lib.WeightedAdamDesc * 1)(_desc(_lib, **kw))
    got = L.et_weighted_adam(_lib.ET_F32, ctypes.addressof(arr), 1, 1e-3, beta[0], beta[1], 1e-8,
                             flags, None, 0, None)
    assert got == rc, L.et_last_error()


def test_call_level_errors_and_workspace():
    from embtab import _lib

    L = _lib.load()

    def call(arr, n, dtype=_lib.ET_F32, ws=None, nbytes=0):
        return L.et_weighted_adam(dtype, ctypes.addressof(arr) if arr is not None else None, n,
                                  1e-3, 0.9, 0.999, 1e-8, 0, ws, nbytes, None)

    one = (_lib.WeightedAdamDesc * 1)(_desc(_lib))
    dtypes = (_lib.ET_I32, 99, _lib.ET_F64, _lib.ET_F16)
    assert [call(one, 1, t) for t in dtypes] == [-4, -4, -3, -3]
    one[0].weights = 8 * P + 4  # aligned for Float32, not for Float64
    assert call(one, 1) == -3 and call(one, 1, _lib.ET_F64) == -1
    assert call(None, 0) == 0 and call(None, 1) == -1 and call(one, -1) == -1
    assert call((_lib.WeightedAdamDesc * 33)(), 33) == -1 and b"32" in L.et_last_error()
    # all three kinds in one call; then table 1's weights inside table 0's first moment
    far = dict(table=9 * P, m=10 * P, v=11 * P, step=12 * P)
    three = (_lib.WeightedAdamDesc * 3)(_desc(_lib, **FIXED), _desc(_lib, weights=13 * P, **far),
                                        _desc(_lib, weights=0, table=14 * P, m=15 * P, v=16 * P,
                                              step=17 * P))
    assert call(three, 3) == -3
    three[1].weights = 5 * P + 128
    assert call(three, 3) == -1 and b"overlap" in L.et_last_error()
    # the size: et_adam_workspace_size plus 16 bytes per occurrence, rounded up to 256
    f, nb, na = L.et_weighted_adam_workspace_size, ctypes.c_int64(-1), ctypes.c_int64(-1)
    assert f(ctypes.addressof(one), 1, None) == -1 and f(None, 1, ctypes.byref(nb)) == -1
    bad = (_lib.WeightedAdamDesc * 1)(_desc(_lib, **dict(FIXED, weights=8 * P)))
    assert f(ctypes.addressof(bad), 1, ctypes.byref(nb)) == -1
    for nnz in (0, 3000):
        d = (_lib.WeightedAdamDesc * 1)(_desc(_lib, nnz=nnz))
        a = (_lib.AdamDesc * 1)(_lib.AdamDesc(*[getattr(d[0], x[0])
                                                for x in _lib.AdamDesc._fields_]))
        assert f(ctypes.addressof(d), 1, ctypes.byref(nb)) == 0
        assert L.et_adam_workspace_size(ctypes.addressof(a), 1, ctypes.byref(na)) == 0
        assert nb.value == na.value + (16 * nnz + 255) // 256 * 256
    # the call's own check is the same carve: one byte short names the number it told
    for base, pad in ((1 << 24, 0), ((1 << 24) + 1, 255)):
        need = nb.value - 256 + pad
        assert call(d, 1, ws=ctypes.c_void_p(base), nbytes=need - 1) == -3
        assert re.search(rb"\b%d bytes" % need, L.et_last_error())


def test_python_binding_takes_weights_with_the_opt_in():
    """An Adam built with weighted=True takes a gradient with weights: on the CPU the call gets
    as far as the device check of the indices.  A default one refuses it as ever."""
    import embtab as et

    A = et.SimpleEmbedding(torch.zeros((10, 16)))
    g = et.SparseEmbeddingUpdate(A.lookup_type, torch.zeros((4, 16)),
                                 torch.ones((4, 2), dtype=torch.int64), torch.ones(8))
    assert et.Adam().weighted is False and et.Adam(weighted=True).weighted is True
    for args in ((A, g), ([A], [g])):
        with pytest.raises(et.ArgumentError, match="device memory"):
            et.update_(et.Adam(weighted=True), *args)
        with pytest.raises(et.ArgumentError, match="weighted gradient"):
            et.update_(et.Adam(), *args)
