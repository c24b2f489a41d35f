"""Float32 tables updated from Float16 / BFloat16 gradients, the parts that need no GPU: the
status codes of ET_FLAG_DELTA_F16 / ET_FLAG_DELTA_BF16 on et_sparse_adagrad and et_sparse_adam
(before any device work), the entries that keep rejecting the two bits, the workspace size,
and what the wrapper still refuses."""
import ctypes

import pytest
import torch

P = 1 << 20  # dummy device addresses: every call below stops at the host checks
F16, BF16 = 2048, 4096
BASE = dict(table=P, ld_table=16, nrows=100, dim=16, pool=4, delta=2 * P, ld_delta=16, idx=3 * P,
            ld_idx=4, batch=8, cols_per_page=0, colptr=0, nnz=0, state=5 * P, ld_state=16,
            m=5 * P, ld_m=16, v=6 * P, ld_v=16, step=7 * P, weights=0)
RAGGED = dict(pool=0, ld_idx=0, colptr=4 * P, nnz=64)


def _arr(S, **kw):
    d = dict(BASE, **kw)
    return (S * 1)(S(*[d[f[0]] for f in S._fields_]))


def _call(L, _lib, entry, arr, dtype, flags):
    a = ctypes.addressof(arr)
    if entry == "adagrad":
        return L.et_sparse_adagrad(dtype, a, 1, 0.1, 1e-8, flags, None, 0, None)
    f = L.et_sparse_adam if entry == "adam" else L.et_weighted_adam
    return f(dtype, a, 1, 1e-3, 0.9, 0.999, 1e-8, flags, None, 0, None)


@pytest.mark.parametrize("entry", ["adagrad", "adam"])
@pytest.mark.parametrize("ragged", [False, True])
def test_flag_status_codes(entry, ragged):
    from embtab import _lib

    L = _lib.load()
    assert (_lib.ET_FLAG_DELTA_F16, _lib.ET_FLAG_DELTA_BF16) == (F16, BF16)
    S = _lib.AdaGradDesc if entry == "adagrad" else _lib.AdamDesc
    kw = RAGGED if ragged else {}
    for flag in (F16, BF16):
        for extra in (0, 1, 512):  # alone, non-temporal, row-wise
            assert _call(L, _lib, entry, _arr(S, **kw), _lib.ET_F32, flag | extra) == -3
        for dtype in (_lib.ET_F64, _lib.ET_F16, _lib.ET_BF16):
            assert _call(L, _lib, entry, _arr(S, **kw), dtype, flag) == -4
        assert _call(L, _lib, entry, _arr(S, ld_delta=15, **kw), _lib.ET_F32, flag) == -1
    assert _call(L, _lib, entry, _arr(S, **kw), _lib.ET_F32, F16 | BF16) == -1
    assert _call(L, _lib, entry, _arr(S, batch=0, **kw), _lib.ET_F32, BF16) == 0  # no work
    # the workspace does not depend on the flag: the size call takes none, and a flagged call
    # asks for the very bytes it names
    size = L.et_adagrad_workspace_size if entry == "adagrad" else L.et_adam_workspace_size
    nb, big = ctypes.c_int64(0), _arr(S, batch=1000, **kw)
    assert size(ctypes.addressof(big), 1, ctypes.byref(nb)) == 0
    for flags in (0, F16, BF16):
        assert _call(L, _lib, entry, _arr(S, batch=1000, **kw), _lib.ET_F32, flags) == -3
        assert b"workspace of %d bytes" % nb.value in L.et_last_error()


def test_other_entries_reject_the_bits():
    from embtab import _lib

    L = _lib.load()
    for flag in (F16, BF16):
        arr = _arr(_lib.WeightedAdamDesc, **RAGGED)
        assert _call(L, _lib, "weighted_adam", arr, _lib.ET_F32, flag) == -1
        assert b"unknown flags" in L.et_last_error()
        wd = dict(BASE, reserved=0, dweights=0, **RAGGED)
        S = _lib.WeightedUpdateDesc
        one = (S * 1)(S(*[wd[f[0]] for f in S._fields_]))
        assert L.et_ragged_sgd_split(_lib.ET_F32, ctypes.addressof(one), 1, 0.1, flag, None, 0,
                                     None) == -4
        assert L.et_ragged_sgd_split(_lib.ET_F32, ctypes.addressof(one), 1, 0.1, 0, None, 0,
                                     None) == -3


def test_wrapper_refusals():
    import embtab as et

    class Dev(torch.Tensor):  # a host tensor that claims to be on the device: checks only
        is_cuda = True

    A = et.SimpleEmbedding(torch.zeros((10, 16)))
    I = torch.ones((4, 2), dtype=torch.int64).as_subclass(Dev)
    g = et.SparseEmbeddingUpdate(A.lookup_type, torch.zeros((4, 16), dtype=torch.bfloat16), I)
    with pytest.raises(NotImplementedError, match="bfloat16 gradient"):
        et.update_(et.Descent(0.1), A, g)
    for opt in (et.Adam(weighted=True), et.AdaGrad(weighted=True)):
        with pytest.raises(et.ArgumentError, match="weighted=True"):
            et.update_(opt, A, g)
    H = et.SimpleEmbedding(torch.zeros((10, 16), dtype=torch.float64))
    with pytest.raises(NotImplementedError, match="float64 table"):
        et.update_(et.Adam(), H, g)
