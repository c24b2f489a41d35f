"""Numpy restatement of the row-wise quantised format (include/embtab.h, "Row-wise quantised
tables"): the quantiser, pack / unpack, dequantisation and the ordered Float32 pooled sum with
16-bit stores.  A helper for tests/test_quant_host.py and tests/test_gpu_quant.py — it holds
no tests.  Only numpy Float32 / Float16 operations, each of them correctly rounded."""
import numpy as np

F32 = np.float32


def payload_bytes(dim, bits):
    return dim * bits // 8


def pack(q, bits):
    """(R, D) integer levels -> (R, D*bits/8) uint8 payload."""
    q = np.asarray(q).astype(np.uint8)
    if bits == 8:
        return q.copy()
    assert q.shape[1] % 2 == 0 and (q < 16).all()
    return (q[:, 0::2] | (q[:, 1::2] << 4)).astype(np.uint8)


def unpack(payload, dim, bits):
    """(R, payload) uint8 -> (R, D) uint8 levels."""
    payload = np.asarray(payload, dtype=np.uint8)
    if bits == 8:
        return payload[:, :dim].copy()
    q = np.empty((payload.shape[0], dim), dtype=np.uint8)
    q[:, 0::2] = payload[:, :dim // 2] & 15
    q[:, 1::2] = payload[:, :dim // 2] >> 4
    return q


def quantize(x, bits):
    """(R, D) Float32 -> (levels (R, D) uint8, scale (R,) float16, bias (R,) float16)."""
    x = np.asarray(x, dtype=F32)
    L = F32(2 ** bits - 1)
    with np.errstate(all="ignore"):
        lo, hi = x.min(axis=1), x.max(axis=1)
        bias = lo.astype(np.float16)
        b = bias.astype(F32)
        scale = ((hi - b) / L).astype(np.float16)
        s = scale.astype(F32)
        bad = ~(np.isfinite(s) & (s > 0))
        scale[bad] = np.float16(1.0)
        s = scale.astype(F32)
        q = np.rint((x - b[:, None]) / s[:, None])  # Float32 ops; rint ties to even
        q = np.minimum(np.maximum(q, F32(0)), L)
        q = np.where(np.isnan(q), F32(0), q)
    return q.astype(np.uint8), scale, bias


def header_bytes(scale, bias):
    """(R, 4) uint8: scale then bias, little-endian Float16."""
    h = np.stack([np.asarray(scale, np.float16), np.asarray(bias, np.float16)], axis=1)
    return np.ascontiguousarray(h).view("<u2").astype("<u2").view(np.uint8).reshape(-1, 4)


def build_rows(x, bits, ld_bytes, split, fill=0):
    """The packed (R, ld_bytes) table (padding = `fill`) and the (R, 4) header array or None."""
    q, scale, bias = quantize(x, bits)
    p = payload_bytes(x.shape[1], bits)
    rows = np.full((x.shape[0], ld_bytes), fill, dtype=np.uint8)
    rows[:, :p] = pack(q, bits)
    h = header_bytes(scale, bias)
    if split:
        return rows, h
    rows[:, p:p + 4] = h
    return rows, None


def split_rows(rows, dim, bits, hdr=None):
    """(levels, scale, bias) of a packed table."""
    p = payload_bytes(dim, bits)
    h = hdr if hdr is not None else rows[:, p:p + 4]
    h = np.ascontiguousarray(h).view(np.float16)
    return unpack(rows[:, :p], dim, bits), h[:, 0].copy(), h[:, 1].copy()


def dequantize(q, scale, bias):
    """v = float(q) * float(scale) + float(bias): the product is exact, the sum rounds once."""
    s = np.asarray(scale, np.float16).astype(F32)[:, None]
    b = np.asarray(bias, np.float16).astype(F32)[:, None]
    return (np.asarray(q).astype(F32) * s + b).astype(F32)


def bf16_rne(x):
    """Float32 -> bfloat16 bits (uint16), round to nearest even; NaN stays NaN."""
    u = np.asarray(x, dtype=F32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    return np.where(np.isnan(x), np.uint16(0x7FC0), r)


def store(acc, out):
    """One conversion of the Float32 sums: 'f32', 'f16' (float16) or 'bf16' (uint16 bits)."""
    if out == "f32":
        return acc.astype(F32)
    if out == "f16":
        with np.errstate(over="ignore"):
            return acc.astype(np.float16)
    return bf16_rne(acc)


def pooled(table, bags, out="f32"):
    """Ordered pooled sum over the dequantised (R, D) Float32 `table`.  `bags` is a (B, P)
    array or a list of 1-D arrays of 1-based indices; an index outside 1..R adds a zero row.
    Returns ((B, D) result, number of out-of-range indices)."""
    R, D = table.shape
    B = len(bags)
    acc = np.zeros((B, D), dtype=F32)
    oob = 0
    zero = np.zeros(D, dtype=F32)
    for j, bag in enumerate(bags):
        for i, r in enumerate(np.asarray(bag).reshape(-1)):
            ok = 1 <= r <= R
            oob += 0 if ok else 1
            v = table[r - 1] if ok else zero
            acc[j] = v if i == 0 else acc[j] + v
    return store(acc, out), oob


def pooled_matrix(table, idx, out="f32"):
    """`pooled` for a (B, P) matrix of IN-RANGE indices, vectorised over the bags."""
    idx = np.asarray(idx)
    if idx.ndim == 1:
        idx = idx[:, None]
    acc = np.zeros((idx.shape[0], table.shape[1]), dtype=F32)
    for i in range(idx.shape[1]):
        v = table[idx[:, i] - 1]
        acc = v.copy() if i == 0 else acc + v
    return store(acc, out)
