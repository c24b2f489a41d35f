"""Numpy restatement of the FP8 row format (include/embtab.h, "FP8 rows"); it holds no tests.
Rows, headers, the pooled sum and the stores are tests/quant_ref.py's; only the codes differ.
Decode goes through torch's CPU float8 views (exact).  Encode clamps to +-FMAX first, then uses
torch's CPU conversion, which rounds to nearest even but does not saturate (57344 becomes NaN
in E4M3).  v is the Float64 q*s + b rounded to Float32: the product has at most 15 significant
bits and the bias 11, so the Float64 sum hides no Float32 tie and v is the one-rounding fma."""
import numpy as np
import torch

import quant_ref as qr

F32 = np.float32
DT = {"e4m3": torch.float8_e4m3fn, "e5m2": torch.float8_e5m2}
FMAX = {"e4m3": F32(448.0), "e5m2": F32(57344.0)}


def decode_table(fmt):
    """The 256 codes as Float32 (NaN / Inf codes included)."""
    return torch.arange(256, dtype=torch.uint8).view(DT[fmt]).to(torch.float32).numpy()


def finite_codes(fmt):
    return np.flatnonzero(np.isfinite(decode_table(fmt))).astype(np.uint8)


def quantize(x, fmt):
    """(R, D) Float32 -> (codes (R, D) uint8, scale (R,) float16, bias (R,) float16)."""
    x = np.asarray(x, dtype=F32)
    with np.errstate(all="ignore"):
        lo, hi = x.min(axis=1), x.max(axis=1)
        bias = ((lo + hi) / F32(2)).astype(np.float16)
        b = bias.astype(F32)
        scale = (np.maximum(hi - b, b - lo) / FMAX[fmt]).astype(np.float16)
        s = scale.astype(F32)
        scale[~(np.isfinite(s) & (s > 0))] = np.float16(1.0)
        s = scale.astype(F32)
        c = np.minimum(np.maximum((x - b[:, None]) / s[:, None], -FMAX[fmt]), FMAX[fmt])
    assert c.dtype == F32 and np.isfinite(c).all()
    codes = torch.from_numpy(np.ascontiguousarray(c)).to(DT[fmt]).view(torch.uint8).numpy()
    return codes, scale, bias


def rows_of(codes, scale, bias, ld_bytes, split, fill=0):
    """The packed (R, ld_bytes) table (padding = `fill`) and the (R, 4) header array or None."""
    R, D = codes.shape
    rows = np.full((R, ld_bytes), fill, dtype=np.uint8)
    rows[:, :D] = codes
    h = qr.header_bytes(scale, bias)
    if split:
        return rows, h
    rows[:, D:D + 4] = h
    return rows, None


def dequantize(codes, scale, bias, fmt):
    q = decode_table(fmt)[codes].astype(np.float64)
    s = np.asarray(scale, np.float16).astype(np.float64)[:, None]
    b = np.asarray(bias, np.float16).astype(np.float64)[:, None]
    return (q * s + b).astype(F32)
