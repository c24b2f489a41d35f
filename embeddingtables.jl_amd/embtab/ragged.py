"""Variable-length bags: ``RaggedIndices(values, colptr)``.

The reference has no ragged form (its pooled lookup takes a dense ``P x B`` matrix); this is
the pattern of a Julia ``SparseMatrixCSC``: ``values`` is ``rowval`` (every bag's indices back
to back, Int64 and 1-based) and ``colptr`` has ``B + 1`` entries, 1-based and non-decreasing;
bag ``j`` (0-based) owns ``values[colptr[j]-1 : colptr[j+1]-1]``.  The pooled sum of a bag is
the reference's (src/lookup.jl:134-147): a copy of the first row, then the others added in
index order; an empty bag is ``zero(T)``.

``values.numel()`` is a CAPACITY: the kernels find a bag from ``colptr`` alone and use the
capacity only to clamp, so both tensors may be refilled in place (also between replays of a
captured HIP graph) with any total length that fits.
"""
from __future__ import annotations

import torch

from . import _lib
from .tables import ArgumentError


class RaggedIndices:
    """``values`` (1-D int64, contiguous) and ``colptr`` (1-D int64, contiguous, ``B + 1``
    entries) on one device.  ``check=True`` also verifies on the device that ``colptr`` starts
    at 1 or more, never decreases and ends within the capacity, and that every value a bag
    covers lies in ``1..maxindex`` when ``maxindex`` is given (one synchronisation)."""

    def __init__(self, values: torch.Tensor, colptr: torch.Tensor, check: bool = False,
                 maxindex: int | None = None):
        for name, x in (("values", values), ("colptr", colptr)):
            if not isinstance(x, torch.Tensor):
                raise TypeError(f"{name} must be an int64 torch tensor")
            if x.dtype != torch.int64:
                raise TypeError(f"{name} must be int64 (Julia Int), got {x.dtype}")
            if x.dim() != 1:
                raise ArgumentError(f"{name} must be 1-D, got {x.dim()} dimensions")
            if x.numel() > 1 and x.stride(0) != 1:
                raise ArgumentError(f"{name} must be contiguous")
        if values.device != colptr.device:
            raise ArgumentError(f"values on {values.device} but colptr on {colptr.device}")
        if colptr.numel() < 1:
            raise ArgumentError("colptr needs batch + 1 entries (at least one)")
        self.values = values
        self.colptr = colptr
        if check:
            self.validate(maxindex)

    @classmethod
    def from_lengths(cls, values: torch.Tensor, lengths, check: bool = False) -> "RaggedIndices":
        """``colptr = 1 + exclusive cumsum(lengths)`` on the device of ``values``."""
        lengths = torch.as_tensor(lengths, dtype=torch.int64, device=values.device).reshape(-1)
        colptr = torch.ones(lengths.numel() + 1, dtype=torch.int64, device=values.device)
        if lengths.numel():
            colptr[1:] += torch.cumsum(lengths, 0)
        return cls(values, colptr, check)

    @property
    def batch(self) -> int:
        return int(self.colptr.numel()) - 1

    @property
    def nnz(self) -> int:
        """The capacity: entries addressable at ``values`` (not the entries in use)."""
        return int(self.values.numel())

    @property
    def device(self):
        return self.values.device

    @property
    def is_cuda(self) -> bool:
        return self.values.is_cuda

    def numel(self) -> int:
        return self.nnz

    def __repr__(self):
        return f"RaggedIndices(batch={self.batch}, nnz={self.nnz}, device={self.device})"

    def lengths(self) -> torch.Tensor:
        return self.colptr[1:] - self.colptr[:-1]

    def clone(self) -> "RaggedIndices":
        return RaggedIndices(self.values.clone(), self.colptr.clone())

    def validate(self, maxindex: int | None = None) -> "RaggedIndices":
        c = self.colptr
        ok = (c[0] >= 1) & (c[-1] - 1 <= self.nnz)
        if c.numel() > 1:
            ok = ok & (c[1:] >= c[:-1]).all()
        if not bool(ok):
            raise ArgumentError("colptr must start at >= 1, never decrease and end within the "
                                "capacity of values")
        if maxindex is not None:
            used = self.values[int(c[0]) - 1:int(c[-1]) - 1]
            if used.numel() and not bool(((used >= 1) & (used <= int(maxindex))).all()):
                raise ArgumentError(f"values outside 1..{int(maxindex)}")
        return self

    def used_range(self) -> tuple[int, int]:
        """0-based ``[lo, hi)`` of the entries the bags cover, clamped to the capacity (one
        synchronisation)."""
        ends = self.colptr[[0, -1]].tolist()
        lo = min(max(ends[0] - 1, 0), self.nnz)
        hi = min(max(ends[1] - 1, lo), self.nnz)
        return lo, hi

    def bag_ids(self) -> torch.Tensor:
        """The 1-based bag of every entry (0 for the capacity tail), et_ragged_bag_ids."""
        if not self.is_cuda:
            raise ArgumentError("indices must be in device memory")
        bag = torch.empty(self.nnz, dtype=torch.int64, device=self.device)
        _lib.check(_lib.load().et_ragged_bag_ids(self.colptr.data_ptr(), self.batch, self.nnz,
                                                 bag.data_ptr(),
                                                 _lib.stream_handle(self.device)))
        return bag


def arithmetic_colptr(batch: int, pool: int, device) -> torch.Tensor:
    """The colptr of a fixed-pool index seen as ragged: ``1 + pool * (0:batch)``."""
    return 1 + pool * torch.arange(batch + 1, dtype=torch.int64, device=device)
