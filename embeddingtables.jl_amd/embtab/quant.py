"""Row-wise quantised tables: INT8 / INT4 rows, or FP8 rows (OCP E4M3FN / E5M2), with a
Float16 scale and bias per row, dequantised inside the pooled sum (include/embtab.h, "Row-wise
quantised tables" and "FP8 rows"; the layout of FBGEMM's Fused8BitRowwise / FusedNBitRowwise
with half-precision headers); or MXFP4 rows (OCP Microscaling FP4: blocks of 32 E2M1 codes under
one E8M0 scale byte, no header and no bias; include/embtab.h, "MXFP4 rows").

A ``QuantizedEmbedding`` is an inference-only table: ``lookup`` / ``maplookup`` and
``PreallocationPlan`` accept it under every strategy (one et_quant_maplookup_prealloc,
et_fp8_maplookup_prealloc or et_mx4_maplookup_prealloc launch per format in the call),
``rrule``, ``update_``, ``PhasedUpdate`` and the sharding classes refuse it.

A table made with ``weighted=True`` (or ``Q.accept_weighted()``) also takes
``WeightedIndices``: per-sample weights and ``mode="mean"``, one
et_quant_weighted_maplookup_prealloc call per format present.  Without the flag such a lookup
raises ``ArgumentError`` as it always did.
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib
from .ragged import RaggedIndices
from .tables import AbstractEmbeddingTable, ArgumentError, Dynamic

OUT_DTYPES = (torch.float32, torch.float16, torch.bfloat16)
# format name -> (launch group: ET_FP8_* of include/embtab.h, 0 for the integer formats, 3 for
# MXFP4; torch's view type of an FP8 code)
FORMATS = {"int": (0, None), "e4m3": (1, torch.float8_e4m3fn), "e5m2": (2, torch.float8_e5m2),
           "mxfp4": (3, None)}
E2M1 = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)  # the magnitude codes; bit 3 is the sign


def check_format(format, bits, dim=None) -> int:
    """The `bits` of a table of `format` (None: the format's own, 4 for MXFP4 and 8 otherwise)."""
    if format not in FORMATS:
        raise ArgumentError(f"format must be 'int', 'e4m3', 'e5m2' or 'mxfp4', got {format!r}")
    if bits is None:
        bits = 4 if format == "mxfp4" else 8
    if format in ("e4m3", "e5m2") and bits != 8:
        raise ArgumentError(f"an FP8 table ({format}) has bits == 8, got {bits!r}")
    if format == "mxfp4":
        if bits != 4:
            raise ArgumentError(f"an MXFP4 table has bits == 4, got {bits!r}")
        if dim is not None and dim % 32:
            raise ArgumentError(f"MXFP4 rows are blocks of 32 features: dim {dim} is no multiple")
    return bits


def payload_bytes(dim: int, bits: int) -> int:
    return dim * bits // 8


def trailer_bytes(dim: int, format: str = "int") -> int:
    """What a fused row carries behind its payload: the 4-byte header, or MXFP4's scale bytes."""
    return dim // 32 if format == "mxfp4" else 4


def split_width(dim: int, format: str = "int") -> int:
    """Bytes per row of the split header array (MXFP4: the scale bytes rounded up to 4)."""
    return (dim // 32 + 3) // 4 * 4 if format == "mxfp4" else 4


def default_ld_bytes(dim: int, bits: int, split_header: bool = False, format: str = "int") -> int:
    """Payload (+ the fused header or scale bytes) rounded up to 16 bytes."""
    n = payload_bytes(dim, bits) + (0 if split_header else trailer_bytes(dim, format))
    return max((n + 15) // 16 * 16, 16)


class QuantizedEmbedding(AbstractEmbeddingTable):
    """``QuantizedEmbedding(packed, dim, bits, header=None, format="int")`` wraps an existing
    packed table.  ``format`` is ``"int"`` (unsigned levels, 8 or 4 bits) or ``"e4m3"`` /
    ``"e5m2"`` (one OCP FP8 code per feature, ``bits == 8``), or ``"mxfp4"`` (``bits == 4``,
    ``dim % 32 == 0``: the rows end in ``dim / 32`` scale bytes instead of the header, and
    ``header`` is the split scale array, ``(R, round_up(dim / 32, 4))`` uint8).

    ``packed`` is a ``(R, ld_bytes)`` uint8 tensor with unit byte stride: row ``r`` holds the
    ``dim * bits / 8`` payload bytes first and, when ``header`` is None, the Float16 scale
    and bias right behind them (the fused header).  ``header`` is a contiguous ``(R, 4)``
    uint8 or ``(R, 2)`` float16 tensor (scale, bias) for the split form.  ``ld_bytes`` (the
    row stride) must be a multiple of 4.  The logical element type is Float32.
    ``weighted=True`` makes the table accept ``WeightedIndices`` (Float32 weights, or
    ``mode="mean"``); it changes nothing about the storage."""

    lookup_type = Dynamic

    def __init__(self, packed: torch.Tensor, dim: int, bits: int,
                 header: torch.Tensor | None = None, format: str = "int",
                 weighted: bool = False):
        if not isinstance(packed, torch.Tensor) or packed.dim() != 2 or packed.dtype != torch.uint8:
            raise ArgumentError("QuantizedEmbedding expects a 2-D (R, ld_bytes) uint8 tensor")
        if isinstance(dim, bool) or not isinstance(dim, int) or dim < 1:
            raise ArgumentError(f"dim must be a positive int, got {dim!r}")
        if bits not in (8, 4):
            raise ArgumentError(f"bits must be 8 or 4, got {bits!r}")
        check_format(format, bits, dim)
        if bits == 4 and dim % 2:
            raise ArgumentError(f"4-bit rows need an even dim, got {dim}")
        if packed.shape[0] < 1:
            raise ArgumentError("a table needs at least one row")
        if packed.shape[1] > 1 and packed.stride(1) != 1:
            raise ArgumentError("the bytes of a row must be contiguous (stride(1) == 1)")
        ld = int(packed.stride(0)) if packed.shape[0] > 1 else int(packed.shape[1])
        need = payload_bytes(dim, bits) + (trailer_bytes(dim, format) if header is None else 0)
        if packed.shape[1] < need:
            raise ArgumentError(f"rows of {packed.shape[1]} bytes hold no {bits}-bit row of dim "
                                f"{dim}{' with its fused header' if header is None else ''} "
                                f"({need} bytes)")
        if ld % 4 or ld < need:
            raise ArgumentError(f"ld_bytes {ld} must be a multiple of 4 and at least {need}")
        if header is not None:
            if format == "mxfp4":
                if not isinstance(header, torch.Tensor) or header.dim() != 2 or \
                        (header.dtype, header.shape[1]) != (torch.uint8, split_width(dim, format)):
                    raise ArgumentError(f"the split scales of an MXFP4 table of dim {dim} are a "
                                        f"(R, {split_width(dim, format)}) uint8 tensor")
            elif not isinstance(header, torch.Tensor) or header.dim() != 2 or \
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
        self.format = format
        self.ld_bytes = ld
        self.weighted = bool(weighted)

    def accept_weighted(self) -> "QuantizedEmbedding":
        """A view of the same storage (no copy) that takes ``WeightedIndices``."""
        return type(self)(self.packed, self.dim, self.bits, self.header, self.format, weighted=True)

    def __repr__(self):
        kind = f"INT{self.bits}" if self.format == "int" else \
            "MXFP4" if self.format == "mxfp4" else f"FP8 {self.format.upper()}"
        return (f"{self.dim}x{self.packed.shape[0]} QuantizedEmbedding{{{kind}, "
                f"{'split' if self.header is not None else 'fused'} header, ld {self.ld_bytes}}}")

    @classmethod
    def quantize(cls, src, bits: int | None = None, ld_bytes: int | None = None,
                 split_header: bool = False, format: str = "int",
                 weighted: bool = False) -> "QuantizedEmbedding":
        """Quantise a Float32 ``(R, D)`` tensor or float table on the device (et_quantize_rows,
        et_fp8_quantize_rows for ``format="e4m3"`` / ``"e5m2"`` or et_mx4_quantize_rows for
        ``"mxfp4"``: include/embtab.h's quantisers).  ``bits`` defaults to the format's own (4 for
        MXFP4, 8 otherwise); ``ld_bytes`` to the payload (+ the header or scale bytes when fused)
        rounded up to 16; padding bytes are zero.  ``weighted``: see the class."""
        bits = check_format(format, bits)
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
        check_format(format, bits, D)
        if D > 1 and src.stride(1) != 1:
            src = src.contiguous()
        need = payload_bytes(D, bits) + (0 if split_header else trailer_bytes(D, format))
        ld = default_ld_bytes(D, bits, split_header, format) if ld_bytes is None else int(ld_bytes)
        if ld % 4 or ld < need:
            raise ArgumentError(f"ld_bytes {ld} must be a multiple of 4 and at least {need}")
        packed = torch.zeros((R, ld), dtype=torch.uint8, device=src.device)
        header = torch.zeros((R, split_width(D, format)), dtype=torch.uint8,
                             device=src.device) if split_header else None
        ld_src = int(src.stride(0)) if R > 1 else D
        hdr = header.data_ptr() if header is not None else None
        L, stream = _lib.load(), _lib.stream_handle(src.device)
        if format == "int":
            _lib.check(L.et_quantize_rows(src.data_ptr(), ld_src, R, D, bits, packed.data_ptr(),
                                          ld, hdr, stream))
        elif format == "mxfp4":
            _lib.check(L.et_mx4_quantize_rows(src.data_ptr(), ld_src, R, D, packed.data_ptr(), ld,
                                              hdr, stream))
        else:
            _lib.check(L.et_fp8_quantize_rows(FORMATS[format][0], src.data_ptr(), ld_src, R, D,
                                              packed.data_ptr(), ld, hdr, stream))
        return cls(packed, D, bits, header, format, weighted=weighted)

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

    def _dequantize_mxfp4(self) -> torch.Tensor:
        """E2M1(q) * 2^(e - 127), exact: the scale is assembled as Float64 bits (e - 127 + 1023
        is a normal exponent for every e), the product is exact in Float64 and every
        representable result converts to Float32 unchanged; e = 255 is NaN."""
        p, nb = self.dim // 2, self.dim // 32
        raw = self.packed[:, :p]
        e = (self.header[:, :nb] if self.header is not None else self.packed[:, p:p + nb])
        e = e.to(torch.int64)
        q = torch.stack((raw & 15, raw >> 4), dim=2).reshape(raw.shape[0], self.dim).to(torch.int64)
        lut = torch.tensor(E2M1 + tuple(-v for v in E2M1), dtype=torch.float64, device=raw.device)
        scale = ((e + (1023 - 127)) << 52).view(torch.float64)
        scale = torch.where(e == 255, torch.full_like(scale, float("nan")), scale)
        return (lut[q] * scale.repeat_interleave(32, dim=1)).to(torch.float32)

    def dequantize(self) -> torch.Tensor:
        """The ``(R, D)`` Float32 table ``q * scale + bias`` (one rounding per element); for
        MXFP4 rows ``E2M1(q) * 2^(e - 127)`` (no rounding)."""
        if self.format == "mxfp4":
            return self._dequantize_mxfp4()
        p = payload_bytes(self.dim, self.bits)
        raw = self.packed[:, :p]
        if self.format != "int":  # the codes' exact Float32 values
            q = raw.contiguous().view(FORMATS[self.format][1]).to(torch.float32)
        elif self.bits == 8:
            q = raw.to(torch.float32)
        else:
            q = torch.stack((raw & 15, raw >> 4), dim=2).reshape(raw.shape[0], self.dim)
            q = q.to(torch.float32)
        h = self._headers().to(torch.float32)
        # the product is exact in Float32 (at most 8 x 11 significant bits), so addcmul's fused
        # or unfused evaluation both round once
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


def quant_descs(tables, Is, B: int, k: int, offs=None):
    """The et_quant_desc arrays of a list of quantised tables (fixed-pool and ragged indices),
    one per format present: what `quant_launch` takes.  `offs` gives every table's first
    destination row (default: back to back from `k`)."""
    from .lookup import _check_idx, _ld, _trailing_size

    descs = (_lib.QuantDesc * len(tables))()
    off = k
    for t, (A, i) in enumerate(zip(tables, Is)):
        if offs is not None:
            off = offs[t]
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
    return quant_groups(tables, descs)


def quant_groups(tables, descs):
    """[(launch group of FORMATS, descriptor array)]: the descriptors of each format present, in
    list order (every descriptor carries its own dst_row_off, so the split changes no result)."""
    fmts = [FORMATS[A.format][0] for A in tables]
    out = []
    for fmt in sorted(set(fmts)):
        pick = [t for t, f in enumerate(fmts) if f == fmt]
        if len(pick) == len(fmts):
            return [(fmt, descs)]
        part = (_lib.QuantDesc * len(pick))()
        for k, t in enumerate(pick):
            part[k] = descs[t]
        out.append((fmt, part))
    return out


def quant_launch(groups, B: int, dst: torch.Tensor, ld_dst: int, flags: int) -> None:
    """et_quant_maplookup_prealloc / et_fp8_maplookup_prealloc / et_mx4_maplookup_prealloc over
    the descriptor groups of `quant_groups`, at most ET_MAX_TABLES_PER_LAUNCH a call."""
    if dst.dtype not in OUT_DTYPES:
        raise ArgumentError(f"a quantised lookup writes Float32, Float16 or BFloat16, not {dst.dtype}")
    L = _lib.load()
    step = _lib.ET_MAX_TABLES_PER_LAUNCH
    size = ctypes.sizeof(_lib.QuantDesc)
    dt, stream = _lib.et_dtype(dst), _lib.stream_handle(dst.device)
    for fmt, descs in groups:
        n = len(descs)
        for c in range(0, n, step):
            part, m = ctypes.addressof(descs) + c * size, min(step, n - c)
            if fmt == 0:
                _lib.check(L.et_quant_maplookup_prealloc(dt, part, m, B, dst.data_ptr(), ld_dst,
                                                         flags, stream))
            elif fmt == FORMATS["mxfp4"][0]:
                _lib.check(L.et_mx4_maplookup_prealloc(dt, part, m, B, dst.data_ptr(), ld_dst,
                                                       flags, stream))
            else:
                _lib.check(L.et_fp8_maplookup_prealloc(dt, fmt, part, m, B, dst.data_ptr(),
                                                       ld_dst, flags, stream))


def quant_weighted_groups(tables, Is, offs, B: int):
    """[(launch group of FORMATS, et_quant_weighted_desc array)] of quantised tables under
    ``WeightedIndices``, one array per format present, every table at its own first destination
    row ``offs[t]``: what `quant_weighted_launch` takes."""
    by = {}
    for t, (A, I, off) in enumerate(zip(tables, Is, offs)):
        if not A.packed.is_cuda or not I.is_cuda:
            raise ArgumentError("the HIP engine needs tables and indices in device memory")
        I.check_for(A)
        if I.batch != B:
            raise ArgumentError(f"table {t}: batch {I.batch} != {B}")
        D, R = A.size()
        r = I.ragged
        desc = _lib.QuantWeightedDesc(
            A.packed.data_ptr(), A.ld_bytes, R, D, A.bits,
            A.header.data_ptr() if A.header is not None else None, r.values.data_ptr(), r.nnz,
            r.colptr.data_ptr(), off, I.weights.data_ptr() if I.weights is not None else None,
            _lib.ET_POOL_MEAN if I.mode == "mean" else _lib.ET_POOL_SUM, 0)
        by.setdefault(FORMATS[A.format][0], []).append(desc)
    return [(fmt, (_lib.QuantWeightedDesc * len(v))(*v)) for fmt, v in sorted(by.items())]


def quant_weighted_launch(groups, B: int, dst: torch.Tensor, ld_dst: int, flags: int) -> None:
    """et_quant_weighted_maplookup_prealloc over the groups of `quant_weighted_groups`, at most
    ET_MAX_TABLES_PER_LAUNCH a call."""
    if dst.dtype not in OUT_DTYPES:
        raise ArgumentError(f"a quantised lookup writes Float32, Float16 or BFloat16, not {dst.dtype}")
    L = _lib.load()
    step, size = _lib.ET_MAX_TABLES_PER_LAUNCH, ctypes.sizeof(_lib.QuantWeightedDesc)
    dt, stream = _lib.et_dtype(dst), _lib.stream_handle(dst.device)
    for fmt, descs in groups:
        for c in range(0, len(descs), step):
            _lib.check(L.et_quant_weighted_maplookup_prealloc(
                dt, fmt, ctypes.addressof(descs) + c * size, min(step, len(descs) - c), B,
                dst.data_ptr(), ld_dst, flags & _lib.ET_FLAG_NONTEMPORAL, stream))
