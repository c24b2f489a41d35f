"""The split sparse SGD over ragged and weighted gradients (et_ragged_sgd_split): the numpy
restatement of the contract in include/embtab.h and the inputs shared by
tests/test_ragged_split_host.py and tests/test_gpu_ragged_split.py.

The gradient sum ``g`` of a column is tests/weighted_adagrad_ref.py's ``weighted_g`` over its
``entry_lists`` (per chunk ``p = +0``, ``t = w_k * delta[bag(k)]``, ``p = p + t``; the partial
sums added in chunk order), or tests/test_gpu_adagrad.py's ``ref_g``, the same rule without a
product, for a table without weights.  The apply step is the arithmetic of
``weighted_ref.sgd`` (``_fma32``, unfused, Float64 alpha); Float64 fused goes through
``oracle.sgd`` over a vector index of the distinct columns with the ``g`` rows as its gradient
(``+0 + g`` is ``g``, so the oracle's fma does the rest)."""
import numpy as np

import test_gpu_adagrad as ta
import weighted_adagrad_ref as war
import weighted_ref as wr

CHUNK = ta.CHUNK
KINDS = ta.KINDS
ROWS = 1000
ETA = 0.1
HOT = 777                                                   # 1-based row of the hot column
FORCED = {601: 255, 602: 256, 603: 257, 604: 512, 605: 513}  # 1-based row: entries
LONELY = 999                                                # named by uncovered entries only
HEAD = 3                                                    # uncovered entries in front


# --- inputs ------------------------------------------------------------------------------------

def split_case(seed, B=300, tail=40):
    """(L, values, colptr).  Mixed lengths with empty bags; ten bags of 300 entries hold the
    hot row (3,000 covered entries; with the HEAD uncovered entries in front that name it as
    well its list has 3,003 positions: 12 chunks, the last holding 187, and every covered
    entry sits HEAD positions later than it would without them); rows with exactly 255, 256,
    257, 512 and 513 entries; the other values from 40 rows below 400; a capacity tail of
    valid indices (LONELY, which no covered entry names, and cold rows)."""
    rng = np.random.default_rng(seed)
    L = wr.mix_lengths(B, rng, extra=[300] * 10 + [200] * 10)
    cp = wr.colptr_of(L)
    used = int(L.sum())
    rows40 = rng.choice(400, 40, replace=False) + 1
    body = rows40[rng.integers(0, 40, used)].astype(np.int64)
    hot_bags = np.nonzero(L == 300)[0][1:]
    assert len(hot_bags) == 10
    is_hot = np.zeros(used, bool)
    for j in hot_bags:
        is_hot[cp[j] - 1:cp[j + 1] - 1] = True
    body[is_hot] = HOT
    cold = rng.permutation(np.nonzero(~is_hot)[0])
    assert len(cold) >= sum(FORCED.values()) + 200
    at = 0
    for row, cnt in FORCED.items():
        body[cold[at:at + cnt]] = row
        at += cnt
    tl = rows40[rng.integers(0, 40, tail)].astype(np.int64)
    tl[::5] = LONELY
    values = np.concatenate([np.full(HEAD, HOT), body, tl]).astype(np.int64)
    colptr = cp + HEAD
    cnt = np.bincount(values, minlength=ROWS + 1)
    assert cnt[HOT] == 3000 + HEAD and all(cnt[r] == c for r, c in FORCED.items())
    assert max(cnt[r] for r in rows40) <= CHUNK
    return L, values, colptr


def case_weights(seed, values, colptr, C):
    """Uniform on [0.25, 2) for covered entries, NaN at every entry no bag covers."""
    return war.case_weights(np.random.default_rng([seed, 1]), values, colptr, C)


# --- the model ---------------------------------------------------------------------------------

def serial_g(deltaC, entries, weights):
    """The serial rule of et_ragged_sgd / et_weighted_sgd: one sum from +0 over the covered
    entries in order."""
    acc = np.zeros(deltaC.shape[1], deltaC.dtype)
    with np.errstate(all="ignore"):
        for b, k in entries:
            if b:
                acc = acc + (deltaC[b - 1] if weights is None else weights[k] * deltaC[b - 1])
    return acc


def chunked_g(deltaC, entries, weights):
    if weights is None:  # no product at all
        with np.errstate(all="ignore"):
            return ta.ref_g(deltaC, [b for b, _ in entries])
    return war.weighted_g(deltaC, entries, weights)


def gradient_sums(kind, delta, values, colptr, weights, nrows=ROWS, nnz=None, serial=False):
    """(entry lists, column -> g in C) of the participating columns."""
    ent = war.entry_lists(values, colptr, nrows, nnz)
    deltaC = kind.toC(delta)
    rule = serial_g if serial else chunked_g
    g_of = {c: rule(deltaC, e, weights) for c, e in ent.items() if any(b for b, _ in e)}
    assert all(g.dtype == kind.C for g in g_of.values())
    return ent, g_of


def apply(kind, table, g_of, eta=ETA, fused=True, f64_alpha=False):
    """sgd_apply_t, in place on `table` (storage type)."""
    bf16 = kind.name == "bf16"
    if not g_of:
        return table
    if kind.name == "f64" and fused:
        import oracle

        cols = np.array(sorted(g_of), np.int64)
        oracle.sgd(table, np.stack([g_of[c] for c in cols]), cols + 1, eta, fused=True)
        return table
    eta_c = wr.convert_eta(table, eta, bf16)
    with np.errstate(all="ignore"):
        for col, g in g_of.items():
            w = kind.toC(table[col])
            if fused:
                assert kind.C is np.float32
                new = wr._fma32(np.full_like(g, -eta_c), g, w)
            elif f64_alpha:
                v = w.astype(np.float64) - np.float64(eta) * g.astype(np.float64)
                new = v.astype(np.float32) if bf16 else v
            else:
                new = w - eta_c * g
            table[col] = wr.from_c(np.asarray(new), table, bf16) if bf16 else new.astype(
                table.dtype)
    return table


def ref_step(kind, table, delta, values, colptr, weights, eta=ETA, fused=True, f64_alpha=False,
             nrows=None, nnz=None, serial=False):
    """The whole update in place; returns (entry lists, g_of)."""
    ent, g_of = gradient_sums(kind, delta, values, colptr, weights,
                              table.shape[0] if nrows is None else nrows, nnz, serial)
    apply(kind, table, g_of, eta, fused, f64_alpha)
    return ent, g_of


# --- launch arithmetic (et_ragged_sgd_split.hip: launch_ragged_sgd_split) --------------------------

def sgd_grid(n):
    return min(max(-(-n // 2048), 256), 16384)


def gpw(cap):
    """Lane groups per wave of the vector kernels at row capacity `cap`."""
    return 64 // (cap // 4) if cap < 256 else 1


def chunk_sweep(n, cap=None):
    """Chunk records one sweep of k_ragged_sgd_chunks<cap> covers (cap None: the generic twin)."""
    return sgd_grid(n) * 4 * (1 if cap is None else gpw(cap))


def combine_sweep(n, cap=None):
    """Multi-chunk columns one sweep of k_ragged_sgd_combine<cap> covers."""
    mmax = n // CHUNK + 2
    if cap is None:
        return min(-(-mmax // 4), 4096) * 4
    return min(-(-mmax // (4 * gpw(cap))), 2048) * 4 * gpw(cap)
