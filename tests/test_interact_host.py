"""et_interact / et_interact_backward without a GPU: the symbols and their prototypes, the
status codes that come before any launch, the wrapper's argument errors, the Julia ccalls."""
import sys

import pytest
import torch

from test_julia_abi import header_functions, jl_class, shim_ccalls

FWD = ["i32", "ptr", "i64", "i64", "i32", "i32", "i32", "ptr", "i64", "u32", "ptr"]
BWD = ["i32", "ptr", "i64", "ptr", "i64", "i64", "i32", "i32", "i32", "ptr", "i64", "u32", "ptr"]


def test_symbols_prototypes_and_julia_tuples():
    from embtab import _lib

    L, decl = _lib.load(), header_functions()
    calls = {name: [jl_class(a) for a in args] for name, _, args in shim_ccalls()}
    for name, classes in (("et_interact", FWD), ("et_interact_backward", BWD)):
        assert name in _lib.EXPORTS and len(getattr(L, name).argtypes) == len(classes)
        assert decl[name] == ("int", classes) and calls[name] == classes
    assert _lib.ET_FLAG_INTERACT_ITSELF == 1024 and _lib.ET_ABI_VERSION == 9


def fwd(L, dtype=0, x=1 << 20, ld_x=24, batch=4, nvec=3, dim=8, copy=8, y=1 << 24, ld_y=11,
        flags=0):
    return L.et_interact(dtype, x, ld_x, batch, nvec, dim, copy, y, ld_y, flags, None)


def bwd(L, dtype=0, nvec=3, dim=8, copy=8, batch=4, flags=0, ld_dx=24):
    return L.et_interact_backward(dtype, 1 << 20, 24, 1 << 22, 11, batch, nvec, dim, copy,
                                  1 << 24, ld_dx, flags, None)


@pytest.mark.parametrize("call", [fwd, bwd])
def test_status_codes_before_any_launch(call):
    """Every call here fails (or is the batch == 0 no-op): the dummy pointers are never used."""
    from embtab import _lib

    L = _lib.load()
    for dtype in (_lib.ET_F64, _lib.ET_I32, _lib.ET_I64, 99):
        assert call(L, dtype=dtype) == -4
    assert call(L, nvec=0) == -4 and call(L, nvec=33) == -4
    assert call(L, dim=6) == -4 and call(L, dtype=_lib.ET_BF16, dim=12) == -4
    assert call(L, dim=1028) == -4 and call(L, flags=2) == -4
    assert call(L, copy=25) == -1 and b"copy" in L.et_last_error()
    assert call(L, copy=-1) == -1 and call(L, batch=-1) == -1
    assert call(L, batch=0) == 0 and call(L, batch=0, flags=1024 | 1) == 0
    assert fwd(L, ld_y=10) == -1 and fwd(L, ld_x=23) == -1 and bwd(L, ld_dx=23) == -1
    assert fwd(L, x=(1 << 20) + 4) == -4 and fwd(L, y=None) == -1
    assert fwd(L, y=(1 << 20) + 32) == -1 and b"overlaps" in L.et_last_error()


def test_wrapper_argument_errors():
    import embtab as et

    X = torch.zeros((4, 24))
    with pytest.raises(et.ArgumentError, match="device memory"):
        et.interact(X, 8)
    with pytest.raises(et.ArgumentError, match="device memory"):
        et.rrule(et.interact, X, 8)
    mod = sys.modules["embtab.interact"]

    class Dev(torch.Tensor):  # a host tensor that claims to be on the device: checks only
        is_cuda = True

    Xd = X.as_subclass(Dev)
    with pytest.raises(et.ArgumentError, match="no multiple"):
        mod._shape(Xd, 7, None, False)
    with pytest.raises(et.ArgumentError, match="stride"):
        mod._shape(torch.zeros((24, 4)).t().as_subclass(Dev), 8, None, False)
    with pytest.raises(et.ArgumentError, match="copy"):
        mod._shape(Xd, 8, 25, False)
    with pytest.raises(et.ArgumentError, match="Float32"):
        mod._shape(X.double().as_subclass(Dev), 8, None, False)
    assert mod._shape(Xd, 8, None, True) == (3, 8, 6, 1024)
    for Y in (torch.zeros((4, 12)), torch.zeros((4, 11), dtype=torch.float16)):
        with pytest.raises(et.ArgumentError, match="Y"):
            et.interact_(Y.as_subclass(Dev), Xd, 8)
