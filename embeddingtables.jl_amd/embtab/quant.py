"""Row-wise quantised tables: INT8 / INT4 rows with a Float16 scale and bias per row,
dequantised inside the pooled sum (include/embtab.h, "Row-wise quantised tables"; the layout
of FBGEMM's Fused8BitRowwise / FusedNBitRowwise with half-precision headers).

A ``QuantizedEmbedding`` is an inference-only table: ``lookup`` / ``maplookup`` and
``PreallocationPlan`` accept it under every strategy (one et_quant_maplookup_prealloc launch
per call), ``rrule``, ``update_``, ``PhasedUpdate`` and the sharding classes refuse it.
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib
from .ragged import RaggedIndices
from .tables import AbstractEmbeddingTable, ArgumentError, Dynamic

OUT_DTYPES = (torch.float32, torch.float16, torch.bfloat16)


def payload_bytes(dim: int, bits: int) -> int:
    return dim * bits // 8


def default_ld_bytes(dim: int, bits: int, split_header: bool = False) -> int:
    """Payload (+ 4 for a fused header) rounded up to 16 bytes."""
    n = payload_bytes(dim, bits) + (0 if split_header else 4)
    return max((n + 15) // 16 * 16, 16)


class QuantizedEmbedding(AbstractEmbeddingTable):
    """``QuantizedEmbedding(packed, dim, bits, header=None)`` wraps an existing packed table.

    ``packed`` is a ``(R, ld_bytes)`` uint8 tensor with unit byte stride: row ``r`` holds the
    ``dim * bits / 8`` payload bytes first and, when ``header`` is None, the Float16 scale
    and bias right behind them (the fused header).  ``header`` is a contiguous ``(R, 4)``
    uint8 or ``(R, 2)`` float16 tensor (scale, bias) for the split form.  ``ld_bytes`` (the
    row stride) must be a multiple of 4.  The logical element type is Float32."""

    lookup_type = Dynamic

    def __init__(self, packed: torch.Tensor, dim: int, bits: int, header: torch.Tensor | None = None):
        if not isinstance(packed, torch.Tensor) or packed.dim() != 2 or packed.dtype != torch.uint8:
            raise ArgumentError("QuantizedEmbedding expects a 2-D (R, ld_bytes) uint8 tensor")
        if isinstance(dim, bool) or not isinstance(dim, int) or dim < 1:
            raise ArgumentError(f"dim must be a positive int, got {dim!r}")
        if bits not in (8, 4):
            raise ArgumentError(f"bits must be 8 or 4, got {bits!r}")
        if bits == 4 and dim % 2:
            raise ArgumentError(f"4-bit rows need an even dim, got {dim}")
        if packed.shape[0] < 1:
            raise ArgumentError("a table needs at least one row")
        if packed.shape[1] > 1 and packed.stride(1) != 1:
            raise ArgumentError("the bytes of a row must be contiguous (stride(1) == 1)")
        ld = int(packed.stride(0)) if packed.shape[0] > 1 else int(packed.shape[1])
        need = payload_bytes(dim, bits) + (4 if header is None else 0)
        if packed.shape[1] < need:
            raise ArgumentError(f"rows of {packed.shape[1]} bytes hold no {bits}-bit row of dim "
                                f"{dim}{' with its fused header' if header is None else ''} "
                                f"({need} bytes)")
        if ld % 4 or ld < need:
            raise ArgumentError(f"ld_bytes {ld} must be a multiple of 4 and at least {need}")
        if header is not None:
            if not isinstance(header, torch.Tensor) or header.dim() != 2 or \
                    (header.dtype, header.shape[1]) not in ((torch.uint8, 4), (torch.float16, 2)):
                raise ArgumentError("header must be a (R, 4) uint8 or (R, 2) float16 tensor")
            if header.shape[0] != packed.shape[0] or not header.is_contiguous():
                raise ArgumentError("header must be contiguous with one entry per row")
            if header.device != packed.device:
                raise ArgumentError("header and packed rows must be on one device")
        self.packed = packed
        self.header = header
        self.dim = dim
        self.bits = bits
        self.ld_bytes = ld

    def __repr__(self):
        return (f"{self.dim}x{self.packed.shape[0]} QuantizedEmbedding{{INT{self.bits}, "
                f"{'split' if self.header is not None else 'fused'} header, ld {self.ld_bytes}}}")

    @classmethod
    def quantize(cls, src, bits: int = 8, ld_bytes: int | None = None,
                 split_header: bool = False) -> "QuantizedEmbedding":
        """Quantise a Float32 ``(R, D)`` tensor or float table on the device
        (et_quantize_rows: include/embtab.h's quantiser).  ``ld_bytes`` defaults to the payload
        (+ 4 when fused) rounded up to 16; padding bytes are zero."""
        if isinstance(src, AbstractEmbeddingTable):
            if isinstance(src, QuantizedEmbedding):
                raise TypeError("QuantizedEmbedding.quantize: the source is already quantised")
            src = src.to_dense() if hasattr(src, "to_dense") else src.example()
        if not isinstance(src, torch.Tensor) or src.dim() != 2:
            raise ArgumentError("quantize expects a (R, D) tensor or a float table")
        if src.dtype != torch.float32:
            raise ArgumentError(f"quantize takes Float32 rows, got {src.dtype}")
        if not src.is_cuda:
            raise ArgumentError("the HIP engine quantises tables in device memory")
        R, D = int(src.shape[0]), int(src.shape[1])
        if bits not in (8, 4):
            raise ArgumentError(f"bits must be 8 or 4, got {bits!r}")
        if R < 1 or D < 1 or (bits == 4 and D % 2):
            raise ArgumentError(f"cannot quantise a {R} x {D} table to {bits} bits")
        if D > 1 and src.stride(1) != 1:
            src = src.contiguous()
        need = payload_bytes(D, bits) + (0 if split_header else 4)
        ld = default_ld_bytes(D, bits, split_header) if ld_bytes is None else int(ld_bytes)
        if ld % 4 or ld < need:
            raise ArgumentError(f"ld_bytes {ld} must be a multiple of 4 and at least {need}")
        packed = torch.zeros((R, ld), dtype=torch.uint8, device=src.device)
        header = torch.zeros((R, 4), dtype=torch.uint8, device=src.device) if split_header else None
        ld_src = int(src.stride(0)) if R > 1 else D
        _lib.check(_lib.load().et_quantize_rows(
            src.data_ptr(), ld_src, R, D, bits, packed.data_ptr(), ld,
            header.data_ptr() if header is not None else None, _lib.stream_handle(src.device)))
        return cls(packed, D, bits, header)

    # --- the table contract -------------------------------------------------------------
    def size(self):
        return (self.dim, int(self.packed.shape[0]))

    @property
    def featuresize(self) -> int:
        return self.dim

    def example(self) -> torch.Tensor:
        return self.packed

    @property
    def dtype(self):
        return torch.float32  # what a lookup produces by default

    def device_table(self):
        raise TypeError("QuantizedEmbedding has no float-table descriptor: it is served by "
                        "lookup / maplookup only (inference only)")

    @property
    def ld(self):
        raise TypeError("QuantizedEmbedding rows are addressed in bytes (ld_bytes)")

    def columnpointer(self, i: int, ctx=None) -> int:
        return self.packed.data_ptr() + (i - 1) * self.ld_bytes

    def _headers(self) -> torch.Tensor:
        """(R, 2) float16: scale, bias."""
        if self.header is not None:
            h = self.header
            return h if h.dtype == torch.float16 else h.view(torch.float16)
        p = payload_bytes(self.dim, self.bits)
        return self.packed[:, p:p + 4].contiguous().view(torch.float16)

    def dequantize(self) -> torch.Tensor:
        """The ``(R, D)`` Float32 table ``q * scale + bias`` (one rounding per element)."""
        p = payload_bytes(self.dim, self.bits)
        raw = self.packed[:, :p]
        if self.bits == 8:
            q = raw.to(torch.float32)
        else:
            q = torch.stack((raw & 15, raw >> 4), dim=2).reshape(raw.shape[0], self.dim)
            q = q.to(torch.float32)
        h = self._headers().to(torch.float32)
        # the product is exact in Float32 (8 x 11 significant bits), so addcmul's fused or
        # unfused evaluation both round once
        return torch.addcmul(h[:, 1:2].expand_as(q), q, h[:, 0:1].expand_as(q))

    def _col(self, j: int) -> torch.Tensor:
        raise TypeError("QuantizedEmbedding elements are read through dequantize()")


def refuse(tables, what: str) -> None:
    """TypeError if a quantised table reaches a training or sharding entry."""
    if isinstance(tables, AbstractEmbeddingTable):
        tables = [tables]
    try:
        tables = list(tables)
    except TypeError:
        return
    for t in tables:
        if isinstance(t, QuantizedEmbedding):
            raise TypeError(f"{what} does not take a QuantizedEmbedding: quantised tables are "
                            "inference only (lookup / maplookup)")


def is_quantized_list(tables) -> bool:
    """True for a list of only quantised tables, False for none; a mix raises."""
    n = sum(isinstance(t, QuantizedEmbedding) for t in tables)
    if n == 0:
        return False
    if n != len(tables):
        raise NotImplementedError(
            "a table list that mixes QuantizedEmbedding and float tables is not one launch: "
            "call maplookup_ twice into one destination, the quantised tables and the float "
            "tables each with their own PreallocationStrategy(prependrows) (the rows before "
            "their block)")
    return True


def quant_descs(tables, Is, B: int, k: int):
    """et_quant_desc array of a list of quantised tables (fixed-pool and ragged indices)."""
    from .lookup import _check_idx, _ld, _trailing_size

    descs = (_lib.QuantDesc * len(tables))()
    off = k
    for t, (A, i) in enumerate(zip(tables, Is)):
        if not A.packed.is_cuda:
            raise ArgumentError("the HIP engine needs tables in device memory")
        _check_idx(i)
        if _trailing_size(i) != B:
            raise ArgumentError(f"table {t}: batch {_trailing_size(i)} != {B}")
        D, R = A.size()
        hdr = A.header.data_ptr() if A.header is not None else None
        if isinstance(i, RaggedIndices):
            descs[t] = _lib.QuantDesc(A.packed.data_ptr(), A.ld_bytes, R, D, A.bits, hdr, 0, 0,
                                      i.values.data_ptr(), 0, i.colptr.data_ptr(), i.nnz, off)
        else:
            pool = 1 if i.dim() == 1 else int(i.shape[1])
            descs[t] = _lib.QuantDesc(A.packed.data_ptr(), A.ld_bytes, R, D, A.bits, hdr, pool, 0,
                                      i.data_ptr(), 1 if i.dim() == 1 else _ld(i), None, 0, off)
        off += D
    return descs


def quant_launch(descs, n: int, B: int, dst: torch.Tensor, ld_dst: int, flags: int) -> None:
    """et_quant_maplookup_prealloc over `n` descriptors, at most ET_MAX_TABLES_PER_LAUNCH a call."""
    if dst.dtype not in OUT_DTYPES:
        raise ArgumentError(f"a quantised lookup writes Float32, Float16 or BFloat16, not {dst.dtype}")
    L = _lib.load()
    step = _lib.ET_MAX_TABLES_PER_LAUNCH
    size = ctypes.sizeof(_lib.QuantDesc)
    for c in range(0, n, step):
        _lib.check(L.et_quant_maplookup_prealloc(
            _lib.et_dtype(dst), ctypes.addressof(descs) + c * size, min(step, n - c), B,
            dst.data_ptr(), ld_dst, flags, _lib.stream_handle(dst.device)))
