"""Weighted and mean-pooled bags: ``WeightedIndices(indices, weights=None, mode="sum")``.

The reference has neither form (``EmbeddingBag``'s ``per_sample_weights`` and
``mode="mean"``); include/embtab.h states the arithmetic.  ``indices`` is a contiguous
``(B, P)`` int64 matrix or a ``RaggedIndices``; a matrix rides in the kernels as the ragged
index it is, with the arithmetic ``colptr`` ``1 + P * (0:B)``.  ``weights`` pairs entry ``k``
of the values with ``weights[k]``; its element type is the accumulator type of the table it
is used with (Float32, or Float64 for Float64 tables), checked at the call.

Forward: ``out = T(w_lo*x_lo + w_(lo+1)*x_(lo+1) + ...)``, every product and every sum
rounded once; without weights the plain ragged sum; ``mode="mean"`` divides the plain sum by
the bag's length.  Backward: the table gradient is a ``SparseEmbeddingUpdate`` that carries
``.weights`` (for mean mode ``1 / len(bag)`` per entry), applied by et_weighted_sgd; with
``weight_grad=True`` the pullback also returns ``dw`` (et_weighted_weight_grad)."""
from __future__ import annotations

import ctypes

import torch

from . import _lib
from .quant import QuantizedEmbedding
from .ragged import RaggedIndices, arithmetic_colptr
from .tables import ArgumentError

MODES = {"sum": _lib.ET_POOL_SUM, "mean": _lib.ET_POOL_MEAN}


def acc_dtype(table_dtype: torch.dtype) -> torch.dtype:
    """The accumulator type C of a table type: the element type of weights and dw."""
    if table_dtype in (torch.float32, torch.float16, torch.bfloat16):
        return torch.float32
    if table_dtype == torch.float64:
        return torch.float64
    raise ArgumentError(f"weighted / mean bags need a floating-point table, got {table_dtype}")


def as_ragged(indices) -> RaggedIndices:
    """``indices`` as the ragged index the weighted kernels walk: a ``RaggedIndices`` as it
    is, a contiguous ``(B, P)`` matrix with the arithmetic colptr."""
    if isinstance(indices, RaggedIndices):
        return indices
    if not isinstance(indices, torch.Tensor) or indices.dtype != torch.int64:
        raise TypeError("indices must be an int64 (B, P) tensor or a RaggedIndices")
    if indices.dim() != 2:
        raise ArgumentError("weighted indices are a (B, P) matrix or a RaggedIndices")
    if not indices.is_contiguous():
        raise ArgumentError("a weighted (B, P) index matrix must be contiguous")
    B, P = int(indices.shape[0]), int(indices.shape[1])
    return RaggedIndices(indices.reshape(-1), arithmetic_colptr(B, P, indices.device))


class WeightedIndices:
    """Indices of a weighted (``weights`` given) or mean-pooled (``mode="mean"``) lookup.
    ``weights`` has the shape of a ``(B, P)`` index matrix or ``(nnz,)``; for a
    ``RaggedIndices`` its length is the capacity of the values, and entries no bag covers are
    never read.  ``weight_grad=True`` makes the pullback of ``rrule`` return ``dw``."""

    def __init__(self, indices, weights: torch.Tensor | None = None, mode: str = "sum",
                 weight_grad: bool = False):
        if mode not in MODES:
            raise ArgumentError(f"mode {mode!r}: 'sum' or 'mean'")
        self.indices = indices
        self.ragged = as_ragged(indices)
        self.mode = mode
        self.weight_grad = bool(weight_grad)
        self.weights = weights
        if weights is None:
            if weight_grad:
                raise ArgumentError("weight_grad=True without weights")
            return
        if mode == "mean":
            raise ArgumentError("mode='mean' takes no weights (as EmbeddingBag)")
        if not isinstance(weights, torch.Tensor):
            raise TypeError("weights must be a torch tensor")
        if weights.dtype not in (torch.float32, torch.float64):
            raise ArgumentError(f"weights are Float32 (Float64 for Float64 tables), got "
                                f"{weights.dtype}")
        nnz = self.ragged.nnz
        shapes = [(nnz,)]
        if isinstance(indices, torch.Tensor):
            shapes.append(tuple(indices.shape))
        if tuple(weights.shape) not in shapes:
            raise ArgumentError(f"weights of shape {tuple(weights.shape)}, expected one of "
                                f"{shapes}")
        if not weights.is_contiguous():
            raise ArgumentError("weights must be contiguous")
        if weights.device != self.ragged.device:
            raise ArgumentError(f"weights on {weights.device} but indices on "
                                f"{self.ragged.device}")

    @property
    def batch(self) -> int:
        return self.ragged.batch

    @property
    def nnz(self) -> int:
        return self.ragged.nnz

    @property
    def device(self):
        return self.ragged.device

    @property
    def is_cuda(self) -> bool:
        return self.ragged.is_cuda

    def numel(self) -> int:
        return self.nnz

    def __repr__(self):
        return (f"WeightedIndices({self.indices if isinstance(self.indices, RaggedIndices) else tuple(self.indices.shape)}, "
                f"weights={'None' if self.weights is None else tuple(self.weights.shape)}, "
                f"mode={self.mode!r})")

    def check_for(self, A) -> None:
        """The table-dependent checks, made at the call."""
        if isinstance(A, QuantizedEmbedding):
            raise ArgumentError("weighted / mean bags over a quantised table are not supported")
        C = acc_dtype(A.dtype)
        if self.weights is not None and self.weights.dtype != C:
            raise ArgumentError(f"weights of {self.weights.dtype} with a {A.dtype} table: they "
                                f"must be {C}")


def weighted_desc(A, I: WeightedIndices, off: int) -> _lib.WeightedDesc:
    I.check_for(A)
    D, R = A.size()
    table, cpp = A.device_table()
    r = I.ragged
    return _lib.WeightedDesc(table, A.ld, R, D, MODES[I.mode], r.values.data_ptr(), r.nnz,
                             r.colptr.data_ptr(), off, cpp,
                             I.weights.data_ptr() if I.weights is not None else None)


def weighted_launch(descs, n: int, B: int, dst: torch.Tensor, ld_dst: int, flags: int) -> None:
    """One et_weighted_maplookup_prealloc call on the current stream."""
    _lib.check(_lib.load().et_weighted_maplookup_prealloc(
        _lib.et_dtype(dst), ctypes.addressof(descs), n, B, dst.data_ptr(), ld_dst,
        flags & _lib.ET_FLAG_NONTEMPORAL, _lib.stream_handle(dst.device)))


def _check_delta(A, delta: torch.Tensor, r: RaggedIndices) -> None:
    D, _ = A.size()
    if delta.dtype != A.dtype:
        raise NotImplementedError(f"a {delta.dtype} gradient of a {A.dtype} table")
    if delta.dim() != 2 or delta.shape[0] != r.batch or delta.shape[1] != D:
        raise ArgumentError(f"gradient shape {tuple(delta.shape)} != ({r.batch}, {D})")
    if delta.numel() > 0 and delta.stride(1) != 1:
        raise ArgumentError("gradient features must be contiguous")


def _ld(x: torch.Tensor) -> int:
    return int(x.stride(0)) if x.shape[0] > 1 else max(int(x.shape[1]), 1)


def weighted_update_desc(A, delta: torch.Tensor, r: RaggedIndices, weights=None,
                         dweights=None) -> _lib.WeightedUpdateDesc:
    if isinstance(A, QuantizedEmbedding):
        raise ArgumentError("weighted gradients of a quantised table are not supported")
    C = acc_dtype(A.dtype)
    _check_delta(A, delta, r)
    for name, w in (("weights", weights), ("dweights", dweights)):
        if w is None:
            continue
        if w.dtype != C or w.numel() != r.nnz or not w.is_contiguous() or w.device != r.device:
            raise ArgumentError(f"{name}: {r.nnz} contiguous {C} entries on {r.device} expected, "
                                f"got {tuple(w.shape)} {w.dtype} on {w.device}")
    D, R = A.size()
    tp, cpp = A.device_table()
    return _lib.WeightedUpdateDesc(tp, A.ld, R, D, 0, delta.data_ptr(), _ld(delta),
                                   r.values.data_ptr(), r.nnz, r.colptr.data_ptr(), r.batch, cpp,
                                   weights.data_ptr() if weights is not None else None,
                                   dweights.data_ptr() if dweights is not None else None)


def weight_grad(A, delta: torch.Tensor, indices, out: torch.Tensor | None = None) -> torch.Tensor:
    """``dw[k] = dot(delta[bag(k)], A[values[k]])`` for every entry (``+0`` where no bag covers
    it), of the accumulator type, read from the table as it is now (et_weighted_weight_grad)."""
    r = as_ragged(indices)
    if not r.is_cuda:
        raise ArgumentError("indices must be in device memory")
    C = acc_dtype(A.dtype)
    dw = out if out is not None else torch.empty(r.nnz, dtype=C, device=r.device)
    descs = (_lib.WeightedUpdateDesc * 1)(weighted_update_desc(A, delta, r, None, dw))
    _lib.check(_lib.load().et_weighted_weight_grad(_lib.TORCH_TO_ET[A.dtype],
                                                   ctypes.addressof(descs), 1,
                                                   _lib.stream_handle(r.device)))
    return dw


def mean_weights(indices, C: torch.dtype) -> torch.Tensor:
    """``1 / len(bag(k))`` for every entry (``0`` where no bag covers it), built on the device
    without a synchronisation: the weights under which the weighted update is the pullback of
    a mean-pooled lookup.  Lengths follow the kernels' clamping rule."""
    r = as_ragged(indices)
    if r.batch == 0 or r.nnz == 0:
        return torch.zeros(r.nnz, dtype=C, device=r.device)
    lo = (r.colptr[:-1] - 1).clamp(0, r.nnz)
    hi = torch.maximum(r.colptr[1:] - 1, lo).clamp(max=r.nnz)
    inv = (hi - lo).clamp(min=1).to(C).reciprocal()
    bag = r.bag_ids()
    return inv[(bag - 1).clamp(min=0)] * (bag > 0).to(C)
