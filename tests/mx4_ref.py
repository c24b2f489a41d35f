"""Numpy restatement of include/embtab.h's "MXFP4 rows"; the pooled sum is quant_ref's."""
import numpy as np

import quant_ref as qr

F32 = np.float32
E2M1 = np.array([0, 0.5, 1, 1.5, 2, 3, 4, 6], np.float64)
TABLE = np.concatenate([E2M1, -E2M1])  # code 8 is -0
pooled, pooled_matrix = qr.pooled, qr.pooled_matrix


def decode(codes, scale_bytes):
    """(R, D) codes, (R, D/32) scale bytes -> Float32: a Float64 ldexp converted once; 255: NaN."""
    e = np.repeat(np.asarray(scale_bytes).astype(np.int64), 32, axis=1)
    with np.errstate(over="ignore"):
        v = np.ldexp(TABLE[codes], e - 127).astype(F32)
    return np.where(e == 255, F32(np.nan), v)


def quantize(x):
    """(R, D) finite Float32 -> (codes (R, D) uint8, scale bytes (R, D/32) uint8)."""
    x = np.asarray(x, F32)
    R, D = x.shape
    b = x.reshape(R, D // 32, 32)
    amax = np.abs(b).max(axis=2)
    e = np.maximum((amax.view(np.uint32) >> 23).astype(np.int64) - 2, 0)
    y = (b.astype(np.float64) * np.ldexp(1.0, 127 - e)[:, :, None]).astype(F32)  # one rounding
    a = np.minimum(np.abs(y), F32(6))
    # nearest, ties to the even code: 0.25 .75 1.25 1.75 2.5 3.5 5 become the values 0 1 1 2 2 4 4
    m = ((a > 0.25).astype(int) + (a >= 0.75) + (a > 1.25) + (a >= 1.75) + (a > 2.5) + (a >= 3.5)
         + (a > 5))
    return (m | (np.signbit(y) << 3)).astype(np.uint8).reshape(R, D), e.astype(np.uint8)


def rows_of(codes, scale_bytes, ld_bytes, split, fill=0):
    """The packed (R, ld_bytes) table and the (R, round_up(D/32, 4)) split scales or None."""
    R, D = codes.shape
    nb = D // 32
    rows = np.full((R, ld_bytes), fill, np.uint8)
    rows[:, :D // 2] = qr.pack(codes, 4)
    if split:
        hdr = np.full((R, (nb + 3) // 4 * 4), fill, np.uint8)
        hdr[:, :nb] = scale_bytes
        return rows, hdr
    rows[:, D // 2:D // 2 + nb] = scale_bytes
    return rows, None


def pinned():
    """Blocks pinned by value: (x (4, 32) Float32, their codes, their scale bytes).  Zeros; one
    spike (3 = 6 * 2^-1); every tie and -0 under scale 1; saturation of (6, 8)."""
    x = np.zeros((4, 32), F32)
    codes = np.zeros((4, 32), np.uint8)
    x[1, 5], codes[1, 5] = 3.0, 7
    t = [6, 0.25, 0.75, 2.5, 5, -0.25, -0.75, -2.5, -5, 1.25, 1.75, 3.5, -0.0]
    x[2, :len(t)], codes[2, :len(t)] = t, [7, 0, 2, 4, 6, 8, 10, 12, 14, 2, 4, 6, 8]
    x[3, :3], codes[3, :3] = [7.5, -7.99, 6.5], [7, 15, 7]
    return x, codes, np.array([[0], [126], [127], [127]], np.uint8)
