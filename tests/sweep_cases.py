"""Case builders and host predicates shared by tests/test_gpu_second_sweep.py,
tests/test_gpu_family_sweep.py and tests/test_family_sweep_host.py.  It holds no tests and no
fixtures, and nothing here touches a device: every builder returns numpy arrays (bfloat16 as
uint16 bit patterns, as everywhere in the suite) and plain Python values.

Three parts:

* the launch thresholds of the update kernels restated on the host (``sgd_grid``,
  ``chunk_groups``, ``combine_groups``, ``BAG_IDS_BAGS``, ``APPLY_COLUMNS``) and the predicates
  that count what a shape puts against them (distinct columns, chunk records, multi-chunk
  columns, non-empty bags beyond a bag number);
* the shapes of the second-sweep tests, each the smallest that crosses its threshold, and the
  AdaGrad reference vectorised across columns of one occurrence count (``equal_count_step``);
* the seeded draws of the family sweeps (``forward_case``, ``update_case``, ``multi_case``).

The second-sweep cases are built once and shared (``lru_cache``): a test copies what it
updates in place.  The helpers of the families' own files are imported at first use (they
import torch)."""
import functools

import numpy as np

import quant_ref as qr
import weighted_ref as wr

CHUNK = 256  # ET_SGD_CHUNK (asserted against the library where a test has it loaded)
MAX_ENTRIES = 60000  # per sweep case: keeps the per-entry Python references cheap


def _ta():
    import test_gpu_adagrad as ta

    return ta


def _war():
    import weighted_adagrad_ref as war

    return war


def kind_of(name):
    """tests/test_gpu_adagrad.py's Kind (storage type, accumulator type, conversions)."""
    return _ta().KINDS["f16" if name == "f16acc" else name]


def colptr_of(L):
    return wr.colptr_of(L)


# --- launch thresholds (the source line of each is in tests/test_gpu_second_sweep.py) -----------

BAG_IDS_BAGS = 16384 * 16   # k_ragged_bag_ids: bags one grid sweep covers
APPLY_COLUMNS = 16384 * 4   # k_ragged_apply / k_weighted_apply: distinct columns per sweep


def cdiv(a, b):
    return -(-a // b)


def sgd_grid(n):
    """et_update.hip sgd_grid: clamp(cdiv(n, 2048), 256, 16384) workgroups."""
    return min(max(cdiv(n, 2048), 256), 16384)


def capacity(dim):
    """The vector kernels' capacity of a Float32 table of `dim` (a multiple of 4, at most
    2048): the next of 16, 32, ..., 2048."""
    assert dim % 4 == 0 and 0 < dim <= 2048
    cap = 16
    while cap < dim:
        cap *= 2
    return cap


def gpw(cap):
    """Lane groups per wave: 64 / (D / 4) for capacity D < 256, 1 otherwise and generic."""
    return 64 // (cap // 4) if cap is not None and cap // 4 < 64 else 1


def chunk_groups(n, cap):
    """Lane groups of k_adagrad_chunks<cap> (cap None: the generic twin, one wave a group)
    for a call of `n` occurrences: grid * 4 * GPW."""
    return sgd_grid(n) * 4 * gpw(cap)


def combine_groups(n, cap):
    """Lane groups of k_adagrad_combine<cap> (cap None: generic): the grid is
    cdiv(n / CHUNK + 2, 4 * GPW) workgroups, capped at 2048 (4096 generic)."""
    g = gpw(cap)
    return min(cdiv(n // CHUNK + 2, 4 * g), 4096 if cap is None else 2048) * 4 * g


# --- host predicates ---------------------------------------------------------------------------

def column_counts(values, nrows):
    """Occurrences of every in-range column (1-based values; index 0 of the result unused)."""
    v = np.asarray(values).reshape(-1)
    v = v[(v >= 1) & (v <= nrows)]
    return np.bincount(v, minlength=nrows + 1)


def distinct_columns(values, nrows):
    return int((column_counts(values, nrows) > 0).sum())


def chunk_records(values, nrows):
    """sum(ceil(count / CHUNK)) over the in-range columns."""
    c = column_counts(values, nrows)
    return int(((c + CHUNK - 1) // CHUNK).sum())


def multi_chunk_columns(values, nrows):
    return int((column_counts(values, nrows) > CHUNK).sum())


def bags_beyond(colptr, first):
    """Non-empty bags whose 0-based number is at least `first`."""
    return int((np.diff(np.asarray(colptr))[first:] > 0).sum())


def crosses_bag_ids(colptr):
    """The bag-id kernel sweeps its grid twice and the second sweep's entries are in use."""
    return len(colptr) - 1 > BAG_IDS_BAGS and bags_beyond(colptr, BAG_IDS_BAGS) >= 20


def crosses_apply(values, nrows):
    return distinct_columns(values, nrows) > APPLY_COLUMNS


def crosses_chunks(values, nrows, cap):
    """More chunk records than lane groups, and records that differ from columns."""
    v = np.asarray(values).reshape(-1)
    return (chunk_records(v, nrows) > chunk_groups(len(v), cap)
            and chunk_records(v, nrows) > distinct_columns(v, nrows))


def crosses_combine(values, nrows, cap):
    v = np.asarray(values).reshape(-1)
    return multi_chunk_columns(v, nrows) > combine_groups(len(v), cap)


# --- 1a. bag ids past one grid sweep -------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def bag_ids_case():
    """One ragged table of 700 columns x dim 16 under 262,144 + 53 bags of 0, 1 or 2 entries:
    the first bag empty, the last non-empty, 27 non-empty bags beyond bag 262,144, a capacity
    tail of 7 valid indices (NaN weights there).  Every column holds about 375 entries."""
    rng = np.random.default_rng(0x1A)
    R, D, B = 700, 16, BAG_IDS_BAGS + 53
    L = rng.integers(0, 3, B).astype(np.int64)
    L[BAG_IDS_BAGS::2] = 1
    L[0], L[-1] = 0, 2
    used = int(L.sum())
    values = rng.integers(1, R + 1, used + 7).astype(np.int64)
    weights = (0.25 + 1.75 * rng.random(used + 7)).astype(np.float32)
    weights[used:] = np.nan
    return {
        "R": R, "D": D, "B": B, "L": L, "used": used, "values": values, "colptr": colptr_of(L),
        "weights": weights, "bag": np.repeat(np.arange(B), L),
        "table": rng.standard_normal((R, D)).astype(np.float32),
        "state": rng.random((R, D)).astype(np.float32),
        "delta": rng.standard_normal((B, D)).astype(np.float32)}


@functools.lru_cache(maxsize=None)
def small_ragged_case():
    """The 301-bag table that rides beside `bag_ids_case` in the two-table calls."""
    rng = np.random.default_rng(0x1A1)
    R, D, B = 700, 16, 301
    L = wr.mix_lengths(B, rng)
    return {
        "R": R, "D": D, "B": B, "L": L, "used": int(L.sum()), "colptr": colptr_of(L),
        "values": rng.integers(1, R + 1, int(L.sum())).astype(np.int64),
        "bag": np.repeat(np.arange(B), L),
        "table": rng.standard_normal((R, D)).astype(np.float32),
        "delta": rng.standard_normal((B, D)).astype(np.float32)}


# --- 1b. apply kernels past one grid sweep -------------------------------------------------------

@functools.lru_cache(maxsize=None)
def apply_case():
    """70,000 columns x dim 16, all of them touched: a permutation of 1..R, then 10,000
    uniform draws, in 20,000 bags of 4."""
    rng = np.random.default_rng(0x1B)
    R, D, P = 70000, 16, 4
    values = np.concatenate([rng.permutation(R) + 1,
                             rng.integers(1, R + 1, 10000)]).astype(np.int64)
    B = len(values) // P
    L = np.full(B, P, np.int64)
    return {
        "R": R, "D": D, "B": B, "L": L, "used": len(values), "values": values,
        "colptr": colptr_of(L), "bag": np.repeat(np.arange(B), L),
        "weights": rng.standard_normal(len(values)).astype(np.float32),
        "table": rng.standard_normal((R, D)).astype(np.float32),
        "delta": rng.standard_normal((B, D)).astype(np.float32)}


# --- 1c. the AdaGrad chunk pass past its lane groups ---------------------------------------------

# name: (element kind, dim, touched columns beside the forced ones, capacity or None = generic)
CHUNK_CASES = {
    "cap128": ("f32", 128, 2100, 128),
    "cap16": ("f32", 16, 16500, 16),
    "cap2048": ("f32", 1504, 1100, 2048),
    "generic_f32": ("f32", 7, 1100, None),
    "generic_bf16": ("bf16", 20, 1100, None),
}
CHUNK_WEIGHTED = ("cap128", "generic_f32", "generic_bf16")
CHUNK_FIRST = 20  # 1-based: columns 20 .. 20 + ncols - 1 are touched at least once


@functools.lru_cache(maxsize=None)
def chunk_case(name):
    """A pool-4 index matrix holding tests/test_gpu_adagrad.py's FORCED columns (1, 255, 256,
    257, 513 and 2,307 occurrences) and `ncols` further columns at least once each, and the
    same occurrences as a ragged index (bags of 0..8 entries, a capacity tail of 7) with
    weights.  Columns 1, 2, 4..9, 15..19 and the last 40 stay untouched."""
    ta, war = _ta(), _war()
    kname, D, ncols, cap = CHUNK_CASES[name]
    kind = kind_of(kname)
    rng = np.random.default_rng([0x1C, D])
    P = 4
    forced = np.concatenate([np.full(c, r) for r, c in ta.FORCED.items()])
    once = np.arange(CHUNK_FIRST, CHUNK_FIRST + ncols)
    extra = rng.choice(once, 400 + (-(len(forced) + ncols)) % P)
    flat = rng.permutation(np.concatenate([forced, once, extra])).astype(np.int64)
    I = flat.reshape(-1, P)
    R = CHUNK_FIRST + ncols + 40
    n = len(flat)
    L = rng.integers(0, 9, n).astype(np.int64)
    cut = int(np.searchsorted(np.cumsum(L), n))
    L = L[:cut + 1]
    L[-1] -= int(L.sum()) - n
    assert L.sum() == n and (L >= 0).all()
    values = np.concatenate([flat, rng.choice(once, 7)]).astype(np.int64)
    colptr = colptr_of(L)
    return {
        "name": name, "kind": kname, "D": D, "R": R, "cap": cap, "P": P, "I": I, "n": n,
        "values": values, "colptr": colptr, "L": L,
        "weights": war.case_weights(rng, values, colptr, kind.C),
        "table": kind.fromf(rng.standard_normal((R, D))),
        "state": rng.random((R, D)).astype(kind.C),
        "state_row": rng.random(R).astype(kind.C),
        "delta": kind.fromf(rng.standard_normal((I.shape[0], D))),
        "delta_ragged": kind.fromf(rng.standard_normal((len(L), D)))}


# --- 1d. the AdaGrad combine pass past its lane groups -------------------------------------------

def combine_case(ncols=8200, count=257, D=256, R=8300, B=4096, kname="f32", seed=0x1D):
    """One ragged gradient in which `ncols` columns occur exactly `count` times each, the
    entries shuffled, in `B` bags of unequal lengths around ncols * count / B."""
    kind = kind_of(kname)
    rng = np.random.default_rng(seed)
    cols = 1 + np.sort(rng.choice(R, ncols, replace=False))
    values = rng.permutation(np.repeat(cols, count)).astype(np.int64)
    n = len(values)
    L = np.full(B, n // B, np.int64)
    L[:n % B] += 1
    half = B // 2
    d = rng.integers(0, max(n // B // 4, 1) + 1, half)
    L[0:2 * half:2] += d
    L[1:2 * half:2] -= d
    assert L.sum() == n and (L >= 0).all()
    return {
        "kind": kname, "D": D, "R": R, "B": B, "count": count, "ncols": ncols, "L": L,
        "values": values, "colptr": colptr_of(L),
        "table": kind.fromf(rng.standard_normal((R, D))),
        "state": rng.random((R, D)).astype(kind.C),
        "delta": kind.fromf(rng.standard_normal((B, D)))}


def bag_of_entries(colptr, nnz):
    """The 1-based bag of every entry of the capacity, 0 for an entry no bag covers (a colptr
    that needs no clamping)."""
    colptr = np.asarray(colptr)
    bag = np.zeros(nnz, np.int64)
    lo, hi = int(colptr[0]) - 1, int(colptr[-1]) - 1
    assert 0 <= lo <= hi <= nnz and (np.diff(colptr) >= 0).all()
    bag[lo:hi] = np.repeat(np.arange(1, len(colptr)), np.diff(colptr))
    return bag


def equal_count_lists(values, colptr, nrows):
    """(cols, bagmat): the touched columns (0-based, increasing) and, per column, the bags of
    its entries in increasing entry number: tests/test_gpu_adagrad.py's ``lists_ragged`` as a
    (columns, count) matrix, for values whose in-range columns all occur equally often."""
    values = np.asarray(values)
    ok = (values >= 1) & (values <= nrows)
    order = np.argsort(values, kind="stable")
    order = order[ok[order]]
    cols, counts = np.unique(values[order], return_counts=True)
    assert len(set(counts.tolist())) == 1, "columns of one occurrence count only"
    bag = bag_of_entries(colptr, len(values))
    return cols - 1, bag[order].reshape(len(cols), int(counts[0]))


def equal_count_g(deltaC, bagmat):
    """``ref_g`` for every column at once: step through the list positions, one
    (columns x D) add of the gathered gradient rows per position (a position whose entry no
    bag covers adds nothing), a new partial sum from +0 every CHUNK positions, the partial sums
    added in chunk order.  Per column these are ref_g's additions in ref_g's order."""
    ncols, count = bagmat.shape
    parts = []
    for c0 in range(0, count, CHUNK):
        p = np.zeros((ncols, deltaC.shape[1]), deltaC.dtype)  # +0
        for j in range(c0, min(c0 + CHUNK, count)):
            b = bagmat[:, j]
            if b.all():
                p = p + deltaC[b - 1]
            else:
                use = b != 0
                p[use] = p[use] + deltaC[b[use] - 1]
        parts.append(p)
    g = parts[0]
    for p in parts[1:]:
        g = g + p
    return g


def equal_count_step(kind, table, state, delta, values, colptr, eta=None, eps=None):
    """tests/test_gpu_adagrad.py's element-wise ``ref_step`` for such values, vectorised
    across the columns; in place on `table` (storage type) and `state` (C)."""
    ta = _ta()
    eta = ta.ETA if eta is None else eta
    eps = ta.EPS if eps is None else eps
    C = kind.C
    cols, bagmat = equal_count_lists(values, colptr, table.shape[0])
    live = bagmat.any(axis=1)  # no participating entry: neither column nor state is written
    cols, bagmat = cols[live], bagmat[live]
    g = equal_count_g(kind.toC(delta), bagmat)
    assert g.dtype == C
    s2 = state[cols] + g * g
    d = np.sqrt(s2) + C(eps)
    w2 = kind.toC(table[cols]) - (C(eta) * g) / d
    assert s2.dtype == C and w2.dtype == C
    state[cols] = s2
    table[cols] = kind.toT(w2)


# --- 2. the family sweeps: shared draws ------------------------------------------------------------

SWEEP_ROWS = (1, 3, 129, 700, 5000)
SWEEP_DIMS = (16, 24, 64, 128, 200, 7, 10)
LAWS = ("zero", "one", "uniform", "fixed", "giant")
STORAGES = ("simple", "paged", "colptr")
FORWARD_SEEDS = range(30)
UPDATE_SEEDS = range(30)
MULTI_SEEDS = range(10)


def draw_lengths(law, B, rng):
    """Bag lengths under one of the laws: all 0, all 1, uniform 0..12, a fixed pool, or
    uniform with one bag of 3,000.  The uniform bound and the pool shrink with B so that a
    case stays within MAX_ENTRIES (B = 20,001: uniform 0..4, pool at most 2)."""
    if law == "zero":
        L = np.zeros(B, np.int64)
    elif law == "one":
        L = np.ones(B, np.int64)
    elif law == "fixed":
        P = int(rng.choice([1, 2, 7, 20]))
        L = np.full(B, max(1, min(P, 50000 // B)), np.int64)
    else:
        hi = min(12, 100000 // B)
        L = rng.integers(0, hi + 1, B).astype(np.int64)
        if law == "giant":
            L[int(rng.integers(0, B))] = 3000
    assert L.sum() <= MAX_ENTRIES
    return L


def draw_indices(rng, n, R, zipf):
    """`n` 1-based indices into R columns, uniform or Zipf over a random ranking."""
    if zipf and R > 1:
        a1 = 1.0 - 1.05
        I = np.floor(((float(R) ** a1 - 1.0) * rng.random(n) + 1.0) ** (1.0 / a1))
        return (rng.permutation(R)[I.clip(1, R).astype(np.int64) - 1] + 1).astype(np.int64)
    return rng.integers(1, R + 1, n).astype(np.int64)


def draw_storage(rng, R):
    st = STORAGES[int(rng.integers(0, 3))]
    return st, int(rng.integers(1, max(2, R) + 1))  # the page size of a paged table


def typed(kind, x, scale=1.0):
    return kind.fromf(scale * x)


# --- 2a. forward ---------------------------------------------------------------------------------------

FAMILIES = ("ragged", "wsum", "wmean", "int8", "int4")
FORWARD_KINDS = {"ragged": ("f32", "f64", "f16", "f16acc", "bf16"),
                 "wsum": ("f32", "f64", "f16", "bf16"), "wmean": ("f32", "f64", "f16", "bf16"),
                 "int8": ("f32", "f16", "bf16"), "int4": ("f32", "f16", "bf16")}
FORWARD_B = (1, 2, 5, 63, 64, 65, 255, 257, 1027, 4097, 20001)
QUANT_REF_MAX_B = 1027  # beyond it the quantised expectation is the C oracle's pooled sum


def quant_min_ld(dim, bits, split):
    n = qr.payload_bytes(dim, bits) + (0 if split else 4)
    return max((n + 3) // 4 * 4, 4)


def forward_case(seed):
    """Everything a forward sweep case is, drawn from ``default_rng(seed)``; the family, the
    element type, the batch and the length law walk their lists with the seed so that 30
    seeds reach every one of them (tests/test_family_sweep_host.py asserts it)."""
    rng = np.random.default_rng(seed)
    f, q = seed % 5, seed // 5
    family = FAMILIES[f]
    kinds = FORWARD_KINDS[family]
    kname = kinds[((1 if len(kinds) == 3 else 3) * q + f) % len(kinds)]
    B = FORWARD_B[seed % len(FORWARD_B)]
    law = LAWS[(f + q) % 5]
    quant = family in ("int8", "int4")
    R = int(rng.choice(SWEEP_ROWS))
    dims = [d for d in SWEEP_DIMS if not (family == "int4" and d % 2)]
    D = int(rng.choice(dims))
    tail = int(rng.choice([0, 7]))
    strided = bool(rng.integers(0, 2))
    L = draw_lengths(law, B, rng)
    used = int(L.sum())
    values = rng.integers(1, R + 1, used + tail).astype(np.int64)
    case = {"seed": seed, "family": family, "kind": kname, "B": B, "law": law, "R": R, "D": D,
            "tail": tail, "strided": strided, "L": L, "used": used, "values": values,
            "colptr": colptr_of(L)}
    if quant:
        bits = 8 if family == "int8" else 4
        split, padded = bool(q % 2), bool((q // 2) % 2)  # the four layouts per family
        x = (rng.standard_normal((R, D)) * rng.choice([1e-3, 0.1, 1.0, 30.0], (R, 1))
             + rng.choice([0.0, 1.0, -100.0], (R, 1))).astype(np.float32)
        ld = quant_min_ld(D, bits, split) + (12 if padded else 0)
        rows, hdr = qr.build_rows(x, bits, ld, split, fill=0xA5)
        case.update(bits=bits, split=split, padded=padded, ld_bytes=ld, rows=rows, hdr=hdr,
                    storage=("split" if split else "fused") + ("_padded" if padded else "_min"),
                    table=qr.dequantize(*qr.split_rows(rows, D, bits, hdr)))
    else:
        kind = kind_of(kname)
        storage, page = draw_storage(rng, R)
        case.update(storage=storage, page=page, table=kind.fromf(rng.standard_normal((R, D))))
        if family == "wsum":
            w = rng.standard_normal(used + tail).astype(kind.C)
            w[used:] = np.nan  # the capacity tail is never read
            case.update(weights=w, weight_grad=bool(rng.integers(0, 2)),
                        delta=kind.fromf(rng.standard_normal((B, D))))
    case["params"] = describe(case)
    return case


def describe(case):
    """The drawn parameters, for assertion messages."""
    keys = ("seed", "family", "opt", "kind", "storage", "page", "R", "D", "B", "law", "tail",
            "strided", "zipf", "fixed", "static", "weight_grad", "used", "k", "n")
    return {k: case[k] for k in keys if k in case}


# --- 2b. update -----------------------------------------------------------------------------------------

OPTIMISERS = ("ragged_sgd", "weighted_sgd", "adagrad", "adagrad_row", "wadagrad", "wadagrad_row")
UPDATE_KINDS = ("f32", "f64", "f16", "bf16")
UPDATE_B = (1, 255, 256, 257, 4095, 4096, 4097, 20001)


def update_case(seed):
    """An update sweep case.  AdaGrad takes a fixed-pool (B, P) gradient in a third of its
    cases (the length law is then the fixed pool) and runs two steps with fresh gradients; the
    16-bit gradients of the SGD are scaled by 0.05, as in the families' own files."""
    rng = np.random.default_rng(1000 + seed)
    o, q = seed % 6, seed // 6
    opt = OPTIMISERS[o]
    kname = UPDATE_KINDS[(q + o) % 4]
    kind = kind_of(kname)
    B = UPDATE_B[seed % len(UPDATE_B)]
    law = LAWS[(o + q) % 5]
    adagrad = "adagrad" in opt
    weighted = opt.startswith("w")
    fixed = adagrad and q % 3 == 0
    if fixed:
        law = "fixed"
    R = int(rng.choice(SWEEP_ROWS))
    D = int(rng.choice(SWEEP_DIMS))
    tail = 0 if fixed else int(rng.choice([0, 7]))
    zipf = bool(rng.integers(0, 2))
    storage, page = draw_storage(rng, R)
    static = bool(rng.integers(0, 2))
    L = draw_lengths(law, B, rng)
    used = int(L.sum())
    values = draw_indices(rng, used + tail, R, zipf)
    steps = 2 if adagrad else 1
    scale = 0.05 if (not adagrad and kname in ("f16", "bf16")) else 1.0
    case = {"seed": seed, "opt": opt, "kind": kname, "B": B, "law": law, "R": R, "D": D,
            "tail": tail, "zipf": zipf, "storage": storage, "page": page, "static": static,
            "fixed": fixed, "P": int(L[0]) if fixed else None, "L": L, "used": used,
            "values": values, "colptr": colptr_of(L), "steps": steps,
            "bag": np.repeat(np.arange(B), L), "rowwise": opt.endswith("_row"),
            "weighted": weighted, "adagrad": adagrad,
            "table": kind.fromf(rng.standard_normal((R, D))),
            "deltas": [kind.fromf(scale * rng.standard_normal((B, D))) for _ in range(steps)]}
    if adagrad:
        case["state"] = rng.random(R if case["rowwise"] else (R, D)).astype(kind.C)
    if weighted:
        w = (0.25 + 1.75 * rng.random(used + tail)).astype(kind.C)
        w[used:] = np.nan
        case["weights"] = w
    case["params"] = describe(case)
    return case


# --- 2c. multi-table ------------------------------------------------------------------------------------

MULTI_PREPEND = (0, 1, 4)
GRADIENTS = ("fixed", "ragged", "weighted")


def multi_case(seed):
    """Two to five tables of one element type whose gradients (fixed-pool, ragged and weighted
    mixed) are column blocks of one (B, k + sum(D)) gradient."""
    rng = np.random.default_rng(2000 + seed)
    kname = UPDATE_KINDS[seed % 4]
    kind = kind_of(kname)
    n = int(rng.integers(2, 6))
    B = int(rng.choice([140, 301, 1027]))
    k = MULTI_PREPEND[seed % 3]
    forms = [GRADIENTS[(seed + t) % 3] for t in range(n)]
    tables = []
    for t in range(n):
        R = int(rng.choice([3, 129, 700]))
        D = int(rng.choice([16, 64, 128, 20, 7]))
        form = forms[t]
        if form == "fixed":
            L = np.full(B, int(rng.choice([1, 4, 6])), np.int64)
        else:
            L = wr.mix_lengths(B, rng) if rng.integers(0, 2) else rng.integers(0, 7, B).astype(
                np.int64)
        used = int(L.sum())
        tail = 0 if form == "fixed" else int(rng.choice([0, 7]))
        values = draw_indices(rng, used + tail, R, bool(rng.integers(0, 2)))
        tab = {"R": R, "D": D, "form": form, "L": L, "used": used, "tail": tail,
               "values": values, "colptr": colptr_of(L), "bag": np.repeat(np.arange(B), L),
               "static": bool(rng.integers(0, 2)),
               "table": kind.fromf(rng.standard_normal((R, D)))}
        if form == "weighted":
            w = (0.25 + 1.75 * rng.random(used + tail)).astype(kind.C)
            w[used:] = np.nan
            tab["weights"] = w
        tables.append(tab)
    dims = [t["D"] for t in tables]
    scale = 0.05 if kname in ("f16", "bf16") else 1.0
    case = {"seed": seed, "kind": kname, "n": n, "B": B, "k": k, "tables": tables,
            "offs": np.cumsum([k] + dims).tolist(),
            "delta": kind.fromf(scale * rng.standard_normal((B, k + sum(dims))))}
    case["params"] = dict(describe(case), forms=forms, rows=[t["R"] for t in tables], dims=dims)
    return case
