"""The DLRM pairwise dot interaction over a concatenated ``maplookup`` result.

``X`` is the ``(B, F * dim)`` matrix a ``PreallocationStrategy(dim)`` ``maplookup`` returns when
every table has feature size ``dim`` and the dense vector sits in the prepended columns: ``F``
vectors of ``dim`` features per sample.  ``interact`` returns ``Y`` of shape ``(B, copy + NP)``:
the first ``copy`` columns of ``X`` (default ``dim``: the dense vector) followed by the strict
lower triangle of the sample's ``F x F`` matrix of dot products, row by row (``NP = F(F-1)/2``;
with ``itself=True`` the diagonal is included and ``NP = F(F+1)/2``).  One et_interact launch
on the matrix units; the backward is one et_interact_backward launch (include/embtab.h,
"Pairwise dot interaction", states the arithmetic).  Float32, Float16 and BFloat16."""
from __future__ import annotations

import torch

from . import _lib
from .tables import ArgumentError

DTYPES = (torch.float32, torch.float16, torch.bfloat16)


def _ld(t: torch.Tensor) -> int:
    return int(t.stride(0)) if t.shape[0] > 1 else int(t.shape[1])


def _check_matrix(t, what: str):
    if not isinstance(t, torch.Tensor) or t.dim() != 2:
        raise ArgumentError(f"{what} must be a 2-D (B, width) tensor")
    if not t.is_cuda:
        raise ArgumentError(f"the HIP engine needs {what} in device memory")
    if t.shape[1] > 1 and t.stride(1) != 1:
        raise ArgumentError(f"the columns of {what} must be contiguous (stride(1) == 1)")
    if t.shape[0] > 1 and t.stride(0) < t.shape[1]:
        raise ArgumentError(f"the rows of {what} overlap (stride(0) < width)")


def _shape(X, dim, copy, itself):
    """(F, copy, NP, flags) of a call, after the checks that need no launch."""
    _check_matrix(X, "X")
    if X.dtype not in DTYPES:
        raise ArgumentError(f"interact takes Float32, Float16 or BFloat16, got {X.dtype}")
    if isinstance(dim, bool) or not isinstance(dim, int) or dim < 1:
        raise ArgumentError(f"dim must be a positive int, got {dim!r}")
    width = int(X.shape[1])
    if width == 0 or width % dim:
        raise ArgumentError(f"the width of X ({width}) is no multiple of dim {dim}")
    F = width // dim
    copy = dim if copy is None else copy
    if isinstance(copy, bool) or not isinstance(copy, int) or not 0 <= copy <= width:
        raise ArgumentError(f"copy must be an int in 0..{width}, got {copy!r}")
    NP = F * (F + 1) // 2 if itself else F * (F - 1) // 2
    return F, copy, NP, (_lib.ET_FLAG_INTERACT_ITSELF if itself else 0)


def interact_(Y: torch.Tensor, X: torch.Tensor, dim: int, copy=None, itself: bool = False):
    """``interact`` into a caller's ``(B, copy + NP)`` view; ``Y``'s row stride is its own, so
    a padded output row (a slice of a wider buffer) works.  Returns ``Y``."""
    F, copy, NP, flags = _shape(X, dim, copy, itself)
    _check_matrix(Y, "Y")
    if Y.dtype != X.dtype or Y.device != X.device:
        raise ArgumentError(f"Y is {Y.dtype} on {Y.device}, X is {X.dtype} on {X.device}")
    if tuple(Y.shape) != (X.shape[0], copy + NP):
        raise ArgumentError(f"Y of shape {tuple(Y.shape)}, expected {(X.shape[0], copy + NP)}")
    if Y.numel():  # F == 1 with copy == 0 has nothing to write
        _lib.check(_lib.load().et_interact(
            _lib.et_dtype(X), X.data_ptr(), _ld(X), int(X.shape[0]), F, dim, copy, Y.data_ptr(),
            _ld(Y), flags, _lib.stream_handle(X.device)))
    return Y


def interact(X: torch.Tensor, dim: int, copy=None, itself: bool = False) -> torch.Tensor:
    """The interaction of ``X`` (see the module text) as a fresh ``(B, copy + NP)`` tensor."""
    _, c, NP, _ = _shape(X, dim, copy, itself)
    Y = torch.empty((X.shape[0], c + NP), dtype=X.dtype, device=X.device)
    return interact_(Y, X, dim, copy, itself)


def interact_backward(X: torch.Tensor, dY: torch.Tensor, dim: int, copy=None,
                      itself: bool = False) -> torch.Tensor:
    """``dX``, a fresh ``(B, F * dim)`` tensor of ``X``'s type: the gradient of ``interact`` at
    ``X`` for the output gradient ``dY``."""
    F, copy, NP, flags = _shape(X, dim, copy, itself)
    _check_matrix(dY, "dY")
    if dY.dtype != X.dtype or dY.device != X.device:
        raise ArgumentError(f"dY is {dY.dtype} on {dY.device}, X is {X.dtype} on {X.device}")
    if tuple(dY.shape) != (X.shape[0], copy + NP):
        raise ArgumentError(f"dY of shape {tuple(dY.shape)}, expected {(X.shape[0], copy + NP)}")
    if not dY.numel():  # F == 1 with copy == 0: Y does not depend on X
        return torch.zeros((X.shape[0], F * dim), dtype=X.dtype, device=X.device)
    dX = torch.empty((X.shape[0], F * dim), dtype=X.dtype, device=X.device)
    _lib.check(_lib.load().et_interact_backward(
        _lib.et_dtype(X), X.data_ptr(), _ld(X), dY.data_ptr(), _ld(dY), int(X.shape[0]), F, dim,
        copy, dX.data_ptr(), F * dim, flags, _lib.stream_handle(X.device)))
    return dX

