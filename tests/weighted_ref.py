"""Weighted and mean-pooled bags: a literal numpy restatement of the semantics in
include/embtab.h — element-wise ``np.float32`` / ``np.float64`` operations in the stated
order, one rounding each.  Not a second implementation of the kernels' geometry: plain loops
over bags and entries.

Tables are numpy arrays of float32 / float64 / float16, or bfloat16 bit patterns (uint16)
with ``bf16=True``, as in the oracle's Python binding.  C is the accumulator type: float32,
or float64 for float64 tables."""
import numpy as np

from oracle import bf16_to_f32, f32_to_bf16


def acc_type(table, bf16=False):
    return np.float64 if (table.dtype == np.float64 and not bf16) else np.float32


def to_c(x, bf16=False):
    """Table elements in the accumulator type (exact)."""
    if bf16:
        return bf16_to_f32(x).reshape(x.shape)
    return x.astype(acc_type(x))


def from_c(a, like, bf16=False):
    """T(acc): one RNE rounding for 16-bit tables, the identity otherwise."""
    if bf16:
        return f32_to_bf16(np.ascontiguousarray(a, np.float32)).reshape(a.shape)
    return a.astype(like.dtype)


def ranges(colptr, nnz):
    """The clamping rule of ragged_range: 0 <= lo <= hi <= nnz; also the bounds moved."""
    out, clamped = [], 0
    for j in range(len(colptr) - 1):
        l, h = int(colptr[j]) - 1, int(colptr[j + 1]) - 1
        lo = min(max(l, 0), nnz)
        hi = min(max(h, lo), nnz)
        clamped += (lo != l) + (hi != h)
        out.append((lo, hi))
    return out, clamped


def _row(table, v, C, bf16):
    """C(x) of 1-based index v: +0 when out of range."""
    if 1 <= v <= table.shape[0]:
        return to_c(table[v - 1], bf16)
    return np.zeros(table.shape[1], C)


def forward(table, values, colptr, weights=None, mode="sum", bf16=False, nnz=None):
    """(out, out-of-range events).  ``weights`` of type C or None; mode 'sum' or 'mean'."""
    assert mode in ("sum", "mean") and not (mode == "mean" and weights is not None)
    C = acc_type(table, bf16)
    nnz = len(values) if nnz is None else nnz
    rg, events = ranges(colptr, nnz)
    acc_out = np.zeros((len(rg), table.shape[1]), C)
    with np.errstate(all="ignore"):
        for j, (lo, hi) in enumerate(rg):
            acc = None
            for k in range(lo, hi):
                v = int(values[k])
                events += not (1 <= v <= table.shape[0])
                x = _row(table, v, C, bf16)
                if weights is not None:
                    assert weights.dtype == C
                    x = weights[k] * x           # one rounding in C
                acc = x if acc is None else acc + x  # one rounding in C
            if acc is None:
                continue                          # an empty bag: +0
            if mode == "mean":
                acc = acc / C(hi - lo)            # one correctly rounded division
            acc_out[j] = acc
    return from_c(acc_out, table, bf16), int(events)


def weight_grad_f64(table, delta, values, colptr, bf16=False, nnz=None):
    """(ref, mag): dw and sum_f |delta_f * x_f| per entry, evaluated in float64 (longdouble
    for float64 tables); entries no bag covers and out-of-range indices give 0."""
    nnz = len(values) if nnz is None else nnz
    W = np.longdouble if acc_type(table, bf16) == np.float64 else np.float64
    rg, _ = ranges(colptr, nnz)
    ref, mag = np.zeros(nnz, W), np.zeros(nnz, W)
    t, d = to_c(table, bf16).astype(W), to_c(delta, bf16).astype(W)
    for j, (lo, hi) in enumerate(rg):
        for k in range(lo, hi):
            v = int(values[k])
            if 1 <= v <= table.shape[0]:
                p = d[j] * t[v - 1]
                ref[k], mag[k] = p.sum(), np.abs(p).sum()
    return ref, mag


ROWS = 700
# every length at which the vector kernels take another path (tests/test_gpu_ragged.py)
LENMIX = [0, 1, 2, 3, 4, 5, 7, 8, 9, 33, 300]


def mix_lengths(B, rng, extra=()):
    """First and last bag empty, every LENMIX length (and `extra`) at least once."""
    must = LENMIX + list(extra)
    assert B >= len(must) + 2
    L = rng.integers(0, 13, B)
    pos = 1 + rng.permutation(B - 2)[:len(must)]
    L[pos] = must
    L[0] = L[-1] = 0
    return L.astype(np.int64)


def colptr_of(L):
    return np.concatenate([[1], 1 + np.cumsum(L)]).astype(np.int64)


def typed(x, kind):
    """A float array as a table of `kind`: (array, bf16 flag)."""
    if kind == "bf16":
        return f32_to_bf16(x.astype(np.float32)).reshape(x.shape), True
    return x.astype({"f32": np.float32, "f64": np.float64, "f16": np.float16}[kind]), False


def wgrad_case(dim, kind, B=301):
    """The weight-gradient test's inputs (standard normal, so no product underflows):
    (table, delta, values, colptr, bf16)."""
    rng = np.random.default_rng(1000 + dim)
    L = mix_lengths(B, rng)
    values = rng.integers(1, ROWS + 1, int(L.sum())).astype(np.int64)
    table, bf16 = typed(rng.standard_normal((ROWS, dim)), kind)
    delta, _ = typed(rng.standard_normal((B, dim)), kind)
    return table, delta, values, colptr_of(L), bf16


def gamma(n, u):
    return n * u / (1 - n * u)


def expanded_gradient(delta, weights, colptr, nnz, bf16=False):
    """E[k] = fl_C(w_k * C(delta[bag(k)])) for covered entries, and the covered mask."""
    C = weights.dtype.type
    rg, _ = ranges(colptr, nnz)
    E = np.zeros((nnz, delta.shape[1]), C)
    covered = np.zeros(nnz, bool)
    d = to_c(delta, bf16)
    for j, (lo, hi) in enumerate(rg):
        for k in range(lo, hi):
            E[k] = weights[k] * d[j]
            covered[k] = True
    return E, covered


def _fma32(a, b, c):
    """Correctly rounded float32 fma(a, b, c): the product is exact in float64; the sum is
    rounded to odd in float64 (TwoSum gives the error's sign), then once to float32."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    even = (s.view(np.int64) & 1) == 0
    fix = (err != 0) & even & np.isfinite(s)
    s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(np.float32)


def convert_eta(table, eta, bf16=False):
    """convert(T, eta), held in C."""
    if bf16:
        return bf16_to_f32(f32_to_bf16(np.array([eta], np.float32)))[0]
    if table.dtype == np.float16:
        return np.float32(np.float16(eta))
    return table.dtype.type(eta)


def sgd(table, delta, values, colptr, weights, eta, fused=True, f64_alpha=False, bf16=False,
        nnz=None):
    """In place: for every distinct column, acc = +0, then t = C(w_k) * C(delta[:, bag(k)]),
    acc = acc + t over its covered entries in increasing k, then the update of sgd_apply_t.
    16-bit and float32 tables (float64 fused needs a float64 fma: the oracle pins those)."""
    C = acc_type(table, bf16)
    nnz = len(values) if nnz is None else nnz
    E, covered = expanded_gradient(delta, weights, colptr, nnz, bf16)
    eta_c = convert_eta(table, eta, bf16)
    with np.errstate(all="ignore"):
        for r in np.unique(values[:nnz][covered]):
            if not 1 <= r <= table.shape[0]:
                continue
            acc = np.zeros(table.shape[1], C)
            for k in np.nonzero((values[:nnz] == r) & covered)[0]:
                acc = acc + E[k]
            w = to_c(table[r - 1], bf16)
            if fused:
                assert C == np.float32
                new = _fma32(np.full_like(acc, -eta_c), acc, w)
            elif f64_alpha:
                v = w.astype(np.float64) - np.float64(eta) * acc.astype(np.float64)
                new = v.astype(np.float32) if bf16 else v
            else:
                new = w - eta_c * acc
            table[r - 1] = from_c(np.asarray(new), table, bf16) if bf16 else new.astype(
                table.dtype)
    return table
