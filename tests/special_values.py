"""Special values for the parity tests: Inf, NaN, subnormals, signed zeros and values at the
edge of overflow, the comparison that pins them, and the builders of the cases that
tests/test_gpu_special_values.py runs and tests/test_special_values_host.py vets on the CPU.

Plain numpy (torch is never imported here).  bfloat16 arrays are uint16 bit patterns, as in
the oracle's Python binding; wherever an array's element type matters the functions take
``kind`` in "f32" / "f64" / "f16" / "bf16"."""
import numpy as np

# kind -> (numpy dtype of the array, unsigned type of its bits, exponent bits, mantissa bits)
_FMT = {"f32": (np.float32, np.uint32, 8, 23), "f64": (np.float64, np.uint64, 11, 52),
        "f16": (np.float16, np.uint16, 5, 10), "bf16": (np.uint16, np.uint16, 8, 7)}


def _from_bits(kind, bits):
    dt, ut, _, _ = _FMT[kind]
    return np.asarray(bits, ut).view(dt)


def bits_of(a, kind):
    return np.ascontiguousarray(a).view(_FMT[kind][1])


def palette(kind):
    """Named special values of `kind` (0-d arrays of the array type) and the pairs whose sum
    matters as (a, b, name of a + b)."""
    _, ut, e, m = _FMT[kind]
    sign = 1 << (e + m)
    inf = ((1 << e) - 1) << m
    pos = {"zero": 0, "min_sub": 1, "max_sub": (1 << m) - 1, "min_normal": 1 << m,
           "max": inf - 1, "inf": inf, "one": ((1 << (e - 1)) - 1) << m}
    v = {}
    for name, b in pos.items():
        v[name] = _from_bits(kind, b)
        if name != "one":
            v["-" + name] = _from_bits(kind, b | sign)
    v["nan"] = _from_bits(kind, inf | (1 << (m - 1)))  # quiet, positive, no payload
    pairs = [("max", "max", "inf"), ("min_normal", "-max_sub", "min_sub"),
             ("inf", "-inf", "nan"), ("one", "-one", "zero"), ("-zero", "-zero", "-zero")]
    v["-one"] = _from_bits(kind, pos["one"] | sign)
    if kind == "f16":
        # 40000 + 40000 = 80000 is finite in Float32 and Inf in Float16: in Julia arithmetic
        # [big, big, -big] is Inf, with fp32 accumulation it is 40000 (one final rounding)
        v["big"], v["-big"] = np.float16(40000.0), np.float16(-40000.0)
        pairs.append(("big", "big", "inf"))
    return {"values": v, "pairs": pairs}


def feats_for(dim):
    """Features that always carry the planted values: 0, one in the middle, the last; for a
    masked vector dim (20: capacity 32, 16-byte vectors) also the last feature of the full
    power-of-two part and the first of the last valid vector before the masked tail."""
    f = {0, dim // 2, dim - 1}
    if dim == 20:
        f |= {15, 16}
    return sorted(f)


def plant(array, rows, feats, values):
    """array[rows[i], f] = values[i] for every f in feats (in place; returns array)."""
    assert {0, array.shape[1] - 1} <= set(feats) and len(rows) == len(values)
    for r, x in zip(rows, values):
        array[r, feats] = x
    return array


def nan_mask(a, kind):
    _, _, e, m = _FMT[kind]
    b = bits_of(a, kind).astype(np.uint64)
    return (b & np.uint64((1 << (e + m)) - 1)) > np.uint64(((1 << e) - 1) << m)


def same_special(got, want, kind, copy=False):
    """Equal shapes, equal NaN masks and byte equality outside the NaN mask (the sign of Inf
    and of zero and every subnormal bit); with `copy` (pure copies) the whole of
    ``tobytes()``, NaN sign and payload included."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    if copy:
        return got.tobytes() == want.tobytes()
    ng, nw = nan_mask(got, kind), nan_mask(want, kind)
    if not np.array_equal(ng, nw):
        return False
    return np.array_equal(bits_of(got, kind)[~nw], bits_of(want, kind)[~nw])


def census(ref, kind):
    """Counts of NaN, +Inf, -Inf, subnormal and -0 elements of a reference result."""
    _, _, e, m = _FMT[kind]
    b = bits_of(ref, kind).astype(np.uint64)
    sign = np.uint64(1 << (e + m))
    mag = b & (sign - np.uint64(1))
    inf = np.uint64(((1 << e) - 1) << m)
    return {"nan": int((mag > inf).sum()),
            "+inf": int((b == inf).sum()),
            "-inf": int((b == (inf | sign)).sum()),
            "subnormal": int(((mag > 0) & (mag < np.uint64(1 << m))).sum()),
            "-0": int((b == sign).sum())}


def mutations(ref, kind, clean_row):
    """Copies of `ref`, each wrong in one way a kernel can be wrong: name -> array.  A
    mutation the reference has no element for is left out (the census says which)."""
    _, ut, e, m = _FMT[kind]
    pal = palette(kind)["values"]
    b = bits_of(ref, kind)
    sign, inf = ut(1 << (e + m)), ut(((1 << e) - 1) << m)
    mag = b & ut(sign - ut(1))
    out = {}

    def put(name, mask, value_bits):
        if mask.any():
            x = b.copy()
            x[mask] = value_bits[mask] if np.shape(value_bits) == b.shape else value_bits
            out[name] = x.view(ref.dtype)

    put("flush subnormals", (mag > 0) & (mag < ut(1 << m)), b & sign)
    nan = bits_of(pal["nan"], kind).reshape(())
    put("inf to nan", mag == inf, nan)
    put("-0 to +0", b == sign, ut(0))
    one = np.zeros(b.shape, bool)
    one[clean_row] = True
    put("nan a clean row", one, nan)
    first = np.zeros(b.size, bool)
    hit = np.flatnonzero(mag.reshape(-1) == inf)
    if len(hit):
        first[hit[0]] = True
        put("swap one inf's sign", first.reshape(b.shape), b ^ sign)
    return out


# --- element types ------------------------------------------------------------------------

def typed(x, kind):
    """Float64 values as an array of `kind` (one rounding)."""
    from oracle import f32_to_bf16

    if kind == "bf16":
        return f32_to_bf16(np.asarray(x, np.float64).astype(np.float32)).reshape(np.shape(x))
    return np.asarray(x).astype(_FMT[kind][0])


def table_kind(kind):
    """The forward cases' kinds: 'f16acc' is a Float16 table summed in Float32."""
    return "f16" if kind == "f16acc" else kind


def oracle_kw(kind):
    return {"bf16": {"bf16": True}, "f16acc": {"f16_fp32_acc": True}}.get(kind, {})


# --- forward cases -----------------------------------------------------------------------------

N_ORD = 64  # ordinary rows 2 .. 65 (1-based); row 1 and the last row are planted

SPECIALS = ["nan", "inf", "-inf", "max", "-max", "min_sub", "-min_sub", "max_sub", "-max_sub",
            "min_normal", "-zero", "one", "-one"]


def forward_table(kind, dim, seed, nrows=None):
    """(table, rows): 64 ordinary rows and the planted rows.  rows: name -> 1-based row; row 1
    carries NaN and the last row Inf (an out-of-range index clamped to either end of the
    table, or selected by a product, would show).  With `nrows` the table is that long: the
    bags' ordinary rows 2 .. n_ord + 1 (rows["n_ord"]), the planted rows behind them, further
    ordinary rows that no bag reads, and Inf in the last row."""
    tk = table_kind(kind)
    pal = palette(tk)["values"]
    names = SPECIALS + (["big", "-big"] if tk == "f16" else [])
    order = ["nan"] + [n for n in names if n not in ("nan", "inf")] + ["inf"]
    n_ord = N_ORD if nrows is None else min(N_ORD, nrows - len(order))
    n = n_ord + len(order) if nrows is None else nrows
    rng = np.random.default_rng(seed)
    table = typed(rng.standard_normal((n, dim)), tk)
    rows = {"nan": 1, "inf": n}
    for k, name in enumerate(order[1:-1]):
        rows[name] = n_ord + 2 + k
    plant(table, [r - 1 for r in rows.values()], feats_for(dim), [pal[x] for x in rows])
    rows["n_ord"] = n_ord
    return table, rows


def forward_bags(L, rows, nrows, seed, kind="f32"):
    """Indices for bags of the lengths L over a forward_table: (values, colptr, planted bag
    mask, out-of-range events).  Every planted row is first in a bag, later in a bag, alone
    in a bag (where a bag of one entry exists) and next to its cancelling partner in both
    orders (once with -0 rows for the rest of the bag, so that the pair's sum is the result);
    bags of -0 rows only; two hold an out-of-range index (first, and later)."""
    rng = np.random.default_rng(seed)
    L = np.asarray(L, np.int64)
    cp = np.concatenate([[1], 1 + np.cumsum(L)]).astype(np.int64)
    rows = dict(rows)
    n_ord = rows.pop("n_ord")
    values = rng.integers(2, n_ord + 2, int(L.sum())).astype(np.int64)
    planted = np.zeros(len(L), bool)
    free = list(rng.permutation(len(L)))

    def take(minlen, exact=None):
        for j in free:
            if (L[j] == exact) if exact is not None else (L[j] >= minlen):
                free.remove(j)
                planted[j] = True
                return j, int(cp[j]) - 1, int(L[j])
        return None

    def put(entries, where, minlen=None, exact=None, fill=None):
        got = take(minlen or max(len(entries), 1), exact)
        if got is None:
            return False
        _, lo, n = got
        if fill is not None:
            values[lo:lo + n] = fill
        at = lo if where == "first" else lo + n - len(entries)
        values[at:at + len(entries)] = entries
        return True

    pairs = [("max", "max"), ("min_normal", "-max_sub"), ("inf", "-inf"), ("one", "-one"),
             ("-max", "-max"), ("min_sub", "-min_sub")]
    if table_kind(kind) == "f16":
        pairs.append(("big", "big"))
    for name, r in rows.items():
        put([r], "first", minlen=2)
        put([r], "last", minlen=2)
        put([r], "first", exact=1)
    for a, b in pairs:
        for x, y in ((a, b), (b, a)):
            # the rest of the bag -0 rows (the planted features hold the pair's sum itself),
            # then the pair behind ordinary rows
            put([rows[x], rows[y]], "first", fill=rows["-zero"])
            put([rows[x], rows[y]], "last", minlen=3)
    if table_kind(kind) == "f16":
        put([rows["big"], rows["big"], rows["-big"]], "first")
    for n in sorted(set(L[L > 0].tolist()))[:3]:
        put([rows["-zero"]] * n, "first", exact=n)   # -0 + -0 = -0
    put([rows["max_sub"]] * 2, "first", fill=rows["-zero"])
    for n in (33, 300):                              # a later index chunk of a long bag
        got = take(n, exact=n)
        if got is not None:
            values[got[1] + n - 7] = rows["max_sub"]
            values[got[1] + n - 2] = rows["-inf"]
    events = 0
    events += put([0], "first", minlen=2)            # out of range first: the copy of +0
    events += put([nrows + 1], "last", minlen=2)
    events += put([nrows + 1], "first", exact=1)
    return values, cp, planted, events


def forward_ref(oracle, table, values, cp, kind):
    """The oracle's fixed-pool lookups grouped by bag length; an out-of-range index reads a
    row of +0 appended to the table (include/embtab.h: it adds +0)."""
    n = table.shape[0]
    ext = np.concatenate([table, np.zeros((1, table.shape[1]), table.dtype)])
    v = np.where((values < 1) | (values > n), n + 1, values)
    lens = np.diff(cp)
    out = np.zeros((len(lens), table.shape[1]), table.dtype)
    for L in np.unique(lens):
        if L == 0:
            continue
        sel = np.nonzero(lens == L)[0]
        I = np.stack([v[cp[j] - 1:cp[j + 1] - 1] for j in sel])
        out[sel] = oracle.pooled_sum(ext, I, **oracle_kw(kind))
    return out


def forward_case(kind, dim, L, seed, nrows=None):
    table, rows = forward_table(kind, dim, seed, nrows)
    values, cp, planted, events = forward_bags(L, rows, table.shape[0], seed + 1, kind)
    return {"kind": kind, "table": table, "rows": rows, "values": values, "colptr": cp,
            "planted": planted, "events": events}


FWD_B = 301
# (kind, dim) of the fixed-pool cases, each at pools 1, 8 and 20: the vector kernel (16, 128),
# the masked vector kernel (20), the generic kernel (7) and the scalar-addressed 512-byte bag
# loop (128 x 4 bytes, 256 x 2 bytes) in every float type
FIXED_CASES = ([(k, d) for k in ("f32", "f64", "f16", "f16acc", "bf16") for d in (16, 128, 20, 7)]
               + [(k, 256) for k in ("f16", "f16acc", "bf16")])
POOLS = (1, 8, 20)
RAGGED_DIMS = (16, 128, 20, 7)


def fixed_case(kind, dim, P):
    return forward_case(kind, dim, np.full(FWD_B, P), 1000 * dim + 10 * P)


def ragged_case(dim):
    from weighted_ref import mix_lengths

    return forward_case("f32", dim, mix_lengths(FWD_B, np.random.default_rng(301)), 500 + dim)


def is_clean(case, values=None, planted=None):
    """The bags outside `planted` hold ordinary rows only."""
    values = case["values"] if values is None else values
    planted = case["planted"] if planted is None else planted
    cp = case["colptr"]
    return all(((values[cp[j] - 1:cp[j + 1] - 1] >= 2) &
                (values[cp[j] - 1:cp[j + 1] - 1] <= case["rows"]["n_ord"] + 1)).all()
               for j in np.nonzero(~planted)[0])


def forward_weights(case, C, seed):
    """Weights of the accumulator type C for a forward case: standard normal on the clean
    bags, 1 on the planted ones, and 0, -0, Inf, subnormal and NaN on in-range first entries
    of some clean bags of two or more entries (which thereby become planted)."""
    rng = np.random.default_rng(seed)
    cp, planted = case["colptr"], case["planted"].copy()
    L = np.diff(cp)
    w = rng.standard_normal(len(case["values"])).astype(C)
    for j in np.nonzero(planted)[0]:
        w[cp[j] - 1:cp[j + 1] - 1] = 1
    pal = palette("f64" if C == np.float64 else "f32")["values"]
    rows = case["rows"]
    free = [j for j in np.nonzero(~planted & (L >= 2))[0]]
    # (weight, row it meets): 0 * Inf and 0 * NaN are NaN, 0 * x keeps the sign rule,
    # Inf * 0 is NaN, a subnormal weight times 1.0 stays subnormal
    plan = [("zero", "inf"), ("-zero", "one"), ("zero", "-one"), ("inf", "one"),
            ("inf", "-zero"), ("-inf", "one"), ("min_sub", "one"), ("max_sub", "-one"),
            ("nan", "one"), ("zero", "nan"), ("min_normal", "one"), ("max", "max")]
    values = case["values"].copy()
    for (wn, rn), j in zip(plan, free):
        w[cp[j] - 1] = pal[wn]
        values[cp[j] - 1] = rows[rn]
        planted[j] = True
    return w, values, planted


def mean_values(case):
    """A forward case's values with bags of 3 on subnormal rows (1/3 of a subnormal sum)."""
    cp, planted = case["colptr"], case["planted"].copy()
    L = np.diff(cp)
    values = case["values"].copy()
    rows = case["rows"]
    free = [j for j in np.nonzero(~planted & (L == 3))[0]]
    sets = [("min_sub", "min_sub", "min_sub"), ("max_sub", "max_sub", "max_sub"),
            ("max_sub", "-min_sub", "min_normal"), ("max", "max", "-max")]
    for s, j in zip(sets, free):
        values[cp[j] - 1:cp[j] + 2] = [rows[x] for x in s]
        planted[j] = True
    return values, planted


def int_wrap_case(kind, dim=16, B=301, P=8):
    """Int32 / Int64 pooled sums past INT_MAX wrap (Julia, and the GPU): (table, I, want)."""
    dt = np.int32 if kind == "i32" else np.int64
    info = np.iinfo(dt)
    rng = np.random.default_rng(77)
    table = rng.integers(-2 ** 20, 2 ** 20, (N_ORD + 4, dim)).astype(dt)
    table[N_ORD:] = np.array([info.max, info.min, info.max - 5, -1], dt)[:, None]
    I = rng.integers(1, N_ORD + 1, (B, P)).astype(np.int64)
    for j in range(0, 64, 2):
        I[j, rng.integers(0, P, 3)] = rng.integers(N_ORD + 1, N_ORD + 5, 3)
    I[1] = N_ORD + 1  # P * INT_MAX
    want = table[I[:, 0] - 1].copy()
    with np.errstate(over="ignore"):
        for i in range(1, P):
            want = want + table[I[:, i] - 1]  # numpy integer adds wrap
    return table, I, want


# --- sparse SGD, exact mode -----------------------------------------------------------------------

SGD_B, SGD_P, SGD_D = 2048, 64, 128
SGD_SPEC = [(300, 0), (257, 7), (400, 1), (60, 0)]  # (rows, cols per page; 0 contiguous)
SGD_ETA = 4.0   # eta * (max / 2) overflows while the sum does not
CHUNK = 256     # ET_SGD_CHUNK: a column of more occurrences is a chain in the exact mode
COST2 = {0: 9, 1: 17, 2: 21, 3: 22, 4: 38}  # chain_entry_cost2(2^k), et_update.hip
# gradient features, one effect each (features are independent in the column sum)
F_INF, F_INF_NINF, F_NAN, F_SUB, F_OVF, F_MAXMAX = 0, 5, 63, 64, 100, 127
# table-only features (the gradient is ordinary there, or zero at F_ZERO)
F_WINF, F_WSUB, F_ZERO = 10, 11, 12
SGD_RUNS = [(3, 5, 37, 3), (11, 2, 37, 3), (19, 1, 37, 3), (5, 7, 37, 3),
            (9, 3, 37, 3), (1, 13, 37, 3), (6, 6, 37, 3), (2, 10, 37, 3)]


def zipf(R, shape, rng):
    u = rng.random(shape)
    a1 = 1.0 - 1.05
    x = np.floor(((float(R) ** a1 - 1.0) * u + 1.0) ** (1.0 / a1)).clip(1, R).astype(np.int64)
    return (rng.permutation(R)[x - 1] + 1).astype(np.int64)


def chain_shape(I, c):
    """(S, entries, runs) the chain plan gives column c (1-based) of the (B, P) index I: runs
    r_b per bag, entries at S = 2^k are sum ceil(r_b / S), cost entries *
    chain_entry_cost2(S), cheapest first (k_chain_choose)."""
    r = (I == c).sum(1)
    r = r[r > 0]
    E = [int(np.ceil(r / 2 ** k).sum()) for k in range(5)]
    k = min(range(5), key=lambda k: (E[k] * COST2[k], k))
    return 2 ** k, E[k], r


def sgd_case(seed=607):
    """The streamed-loop shape (four tables: contiguous, paged, column-pointer, early-chain
    size) with special values in the gradient of 8 bags and in the tables.

    Per table two reserved columns cA, cB occur in the planted bags only (37 and 3 times
    each: a 296-occurrence chain of S = 8 entries with a run of 5, and a chunk-pass column);
    the planted bags hold nothing but the table's two hottest columns (runs of SGD_RUNS: a
    partial entry at any S > 1) and cA, cB, so four rows per table meet a planted value and
    every other touched row is clean.  Returns a dict of tables, index matrices, the
    (B, 4 * D) gradient, the planted bags and per table its hot / reserved columns."""
    rng = np.random.default_rng(seed)
    B, P, D = SGD_B, SGD_P, SGD_D
    pal = palette("f32")["values"]
    delta = rng.standard_normal((B, D * len(SGD_SPEC))).astype(np.float32)
    bags = np.sort(rng.choice(np.arange(8, B - 8), 8, replace=False))
    tables, idx, cols = [], [], []
    for t, (R, _) in enumerate(SGD_SPEC):
        x = rng.standard_normal((R, D)).astype(np.float32)
        I = zipf(R, (B, P), rng)
        counts = np.bincount(I.ravel(), minlength=R + 1)[1:]
        hot1, hot2 = (np.argsort(-counts)[:2] + 1).tolist()
        cA, cB = (np.argsort(counts)[:2] + 1).tolist()          # the two rarest: reserved
        spare = int(np.argsort(-counts)[2] + 1)
        I[(I == cA) | (I == cB)] = spare
        for b, (r1, r2, rA, rB) in zip(bags, SGD_RUNS):
            row = [hot1] * r1 + [hot2] * r2 + [cA] * rA + [cB] * rB
            row += [hot1] * (P - len(row))
            I[b] = rng.permutation(np.array(row, np.int64))
        # table values: +-Inf and a subnormal under an ordinary sum, -0 and 0 under a zero
        # sum, 0 under the subnormal sum of cB (fma(-eta, acc, 0) is subnormal)
        x[hot1 - 1, F_WINF], x[hot2 - 1, F_WINF] = pal["inf"], pal["-inf"]
        x[cA - 1, F_WSUB], x[cB - 1, F_WSUB] = pal["max_sub"], pal["-min_sub"]
        x[cA - 1, F_ZERO], x[cB - 1, F_ZERO] = pal["-zero"], pal["min_sub"]
        x[cB - 1, F_SUB] = 0.0
        x[cA - 1, F_SUB] = pal["-max_sub"]
        o = t * D
        delta[bags, o + F_ZERO] = 0.0
        delta[bags[0], o + F_INF] = pal["inf"]
        delta[bags[1], o + F_INF_NINF], delta[bags[7], o + F_INF_NINF] = pal["inf"], pal["-inf"]
        delta[bags[2], o + F_NAN] = pal["nan"]
        # subnormals whose sum is normal in cA (296 of them) and subnormal in cB (24), where
        # eta * acc is subnormal too
        delta[bags, o + F_SUB] = rng.integers(1 << 15, 1 << 16, 8).astype(np.uint32).view(
            np.float32)
        delta[bags[3], o + F_MAXMAX], delta[bags[6], o + F_MAXMAX] = pal["max"], pal["max"]
        # cA: acc = 37 * 2^121 is finite and eta * acc is not; the hot columns stay finite
        delta[bags[4], o + F_OVF] = np.float32(2.0 ** 121)
        tables.append(x)
        idx.append(I)
        cols.append({"hot": (hot1, hot2), "cA": cA, "cB": cB})
    return {"tables": tables, "idx": idx, "delta": delta, "bags": bags, "cols": cols}


def sgd_ref(oracle, case, fused):
    out = []
    D = SGD_D
    for t, (x, I) in enumerate(zip(case["tables"], case["idx"])):
        ref = x.copy()
        oracle.sgd(ref, np.ascontiguousarray(case["delta"][:, t * D:(t + 1) * D]), I, SGD_ETA,
                   fused=fused)
        out.append(ref)
    return out


def sgd_planted_rows(case, t):
    c = case["cols"][t]
    return sorted({*c["hot"], c["cA"], c["cB"]})


# --- queued multi-table launch ------------------------------------------------------------------

QUEUED_ROWS = [9000, 8200, 4099, 50]  # two fabric-class and two cache-class tables (x 128 f32)
QUEUED_B, QUEUED_P = 257, 13


def queued_cases():
    return [forward_case("f32", 128, np.full(QUEUED_B, QUEUED_P), 9000 + t, nrows=r)
            for t, r in enumerate(QUEUED_ROWS)]


def zero_row_inputs(case, P):
    """(table with a row of +0 appended, (B, P) indices with the out-of-range ones on it)."""
    t = case["table"]
    n = t.shape[0]
    v = case["values"]
    return (np.concatenate([t, np.zeros((1, t.shape[1]), t.dtype)]),
            np.where((v < 1) | (v > n), n + 1, v).reshape(-1, P))


# --- sparse SGD on ragged bags: every element type, weights ---------------------------------------

HOT_B, HOT_ROWS = 257, 700
H_INF, H_INF_NINF, H_ZERO, H_WINF, H_WSUB = 0, 5, 10, 11, 12  # features; NaN, subnormals and
# max + max take the middle (dim // 2 - 1, dim // 2) and the last feature


def hot_sgd_case(kind, dim, weighted=False, seed=11):
    """The hot_case of tests/test_gpu_weighted.py (257 ragged bags over 40 of 700 rows, one
    row in ten bags of 300 entries: a chain of S = 16 entries with a last run of 12; a second
    row with 100 entries) with special values in the gradients of the hot bags and of four
    short bags rewritten to hold two rows only, the second of which (reserved) occurs nowhere
    else, and in those three table rows.  With `weighted`, weights of the accumulator type:
    standard normal; 0, -0, subnormals and 1 on entries of the short bags; Inf, NaN and -Inf
    (which reach every feature) on a fifth short bag that holds a row of its own."""
    from test_gpu_weighted import hot_case

    rng = np.random.default_rng(seed)
    pal = palette(kind)["values"]
    L, values, rows40 = hot_case(HOT_B, rng)
    cp = np.concatenate([[1], 1 + np.cumsum(L)]).astype(np.int64)
    hot, second, reserved, victim = (int(r) for r in rows40[:4])
    values[(values == reserved) | (values == victim)] = rows40[4]
    hot_bags = np.nonzero(L == 300)[0][1:]
    short = [j for j in np.nonzero((L >= 4) & (L <= 12))[0] if j not in hot_bags][:5]
    for j in short[:4]:
        n = int(L[j])
        values[cp[j] - 1:cp[j + 1] - 1] = [second] * (n // 2) + [reserved] * (n - n // 2)
    # a row of its own for the weights that reach every feature (Inf, NaN)
    values[cp[short[4]] - 1:cp[short[4] + 1] - 1] = victim
    short, vbag = short[:4], short[4]
    table = typed(rng.standard_normal((HOT_ROWS, dim)), kind)
    delta = typed(rng.standard_normal((HOT_B, dim)), kind)
    mid = dim // 2
    bags = np.concatenate([hot_bags[:3], short, [vbag]]).astype(np.int64)
    delta[hot_bags[0], H_INF] = pal["inf"]
    delta[hot_bags[0], H_INF_NINF], delta[hot_bags[2], H_INF_NINF] = pal["inf"], pal["-inf"]
    delta[short[0], H_INF_NINF], delta[short[3], H_INF_NINF] = pal["-inf"], pal["-inf"]
    delta[short[1], mid - 1] = pal["nan"]
    delta[bags, H_ZERO] = pal["zero"]
    for j in short:                              # subnormals only: the reserved row's sum
        delta[j, mid] = _from_bits(kind, int(rng.integers(1, 1 << (_FMT[kind][3] - 5))))
    delta[short[0], dim - 1], delta[short[2], dim - 1] = pal["max"], pal["max"]
    delta[hot_bags[1], dim - 1] = pal["max"]     # 300 x max in one bag
    for r, x in ((hot, "inf"), (second, "-inf")):
        table[r - 1, H_WINF] = pal[x]
    table[reserved - 1, H_ZERO], table[second - 1, H_ZERO] = pal["-zero"], pal["min_sub"]
    table[reserved - 1, H_WSUB], table[hot - 1, H_WSUB] = pal["-max_sub"], pal["max_sub"]
    table[reserved - 1, mid] = pal["zero"]
    case = {"kind": kind, "table": table, "delta": delta, "L": L, "values": values, "colptr": cp,
            "planted_rows": sorted([hot, second, reserved, victim]), "bags": bags,
            "weights": None}
    if weighted:
        C = np.float64 if kind == "f64" else np.float32
        wp = palette("f64" if kind == "f64" else "f32")["values"]
        w = rng.standard_normal(len(values)).astype(C)
        for j, names in zip(short, (("zero", "-zero"), ("min_sub", "max_sub"), ("-zero", "one"),
                                    ("one", "min_sub"))):
            w[cp[j] - 1], w[cp[j + 1] - 2] = wp[names[0]], wp[names[1]]
        w[cp[vbag] - 1:cp[vbag] + 2] = [wp["inf"], wp["nan"], wp["-inf"]]
        case["weights"] = w
    return case


def hot_sgd_ref(oracle, case, fused, f16_fp32_acc=False):
    """oracle.sgd on the expanded gradient (for weighted 16-bit tables weighted_ref.sgd: the
    oracle takes gradients of the table's type, the expanded one is Float32)."""
    import weighted_ref as wr

    kind, w = case["kind"], case["weights"]
    ref = case["table"].copy()
    bag = np.repeat(np.arange(HOT_B), case["L"])
    if w is None:
        oracle.sgd(ref, case["delta"][bag], case["values"], 0.1, fused=fused,
                   bf16=kind == "bf16", f16_fp32_acc=f16_fp32_acc)
    elif kind in ("f32", "f64"):
        with np.errstate(all="ignore"):
            E, cov = wr.expanded_gradient(case["delta"], w, case["colptr"], len(case["values"]))
        oracle.sgd(ref, E[cov], case["values"][cov], 0.1, fused=fused)
    else:
        with np.errstate(all="ignore"):
            wr.sgd(ref, case["delta"], case["values"], case["colptr"], w, 0.1, fused=fused,
                   bf16=kind == "bf16")
    return ref


# --- AdaGrad ---------------------------------------------------------------------------------------

ADA_COLS = [1, 2, 4, 6, 7, 8, 9, 15]  # 1-based columns the ordinary indices never hold


def adagrad_case(name, dim, ragged=False, rowwise=False, seed=21, plain=False):
    """The AdaGrad tests' inputs (tests/test_gpu_adagrad.py: 300 columns; pool 4 x batch 1024,
    or its ragged case of 301 bags) with eight bags rewritten to one dedicated column each:
      1  state 0 and gradient 0: the update divides by eps alone
      2  state 0 and subnormal gradients, whose squares underflow
      4  state = max finite and gradients of +-2^60: state + g^2 is Inf, the step g / Inf = 0,
         so the row (subnormals, -0 and ordinary values) stays as it is
      6, 7, 8  +Inf, NaN and -Inf gradients at the planted features
      9  +-Inf table elements under ordinary gradients
      15 a subnormal state under a zero gradient
    Returns table, state (C; a vector when row-wise), delta, the index (I, or values and
    colptr), the occurrence lists and the planted columns (0-based).  `plain`: the same
    indices with ordinary values everywhere (what the clean columns must not differ from)."""
    import test_gpu_adagrad as ta

    kind = ta.KINDS[name]
    tk = "bf16" if name == "bf16" else name
    pal, palC = palette(tk)["values"], palette("f64" if name == "f64" else "f32")["values"]
    rng = np.random.default_rng([seed, dim, int(ragged), int(rowwise)])
    table = kind.fromf(rng.standard_normal((ta.R, dim)))
    state = rng.random(ta.R if rowwise else (ta.R, dim)).astype(kind.C)
    feats = feats_for(dim)
    if ragged:
        L, values, colptr = ta.ragged_case(rng)
        nb = len(L)
        first = np.nonzero(L > 0)[0][0]
        pick = [j for j in np.nonzero((L >= 2) & (L <= 12))[0] if j != first][:8]
        for j, c in zip(pick, ADA_COLS):
            values[colptr[j] - 1:colptr[j + 1] - 1] = c
        index = (values, colptr)
        lists = ta.lists_ragged(values, colptr)
    else:
        I = ta.make_indices(rng)
        nb = ta.B
        pick = rng.choice(nb, 8, replace=False)
        for j, c in zip(pick, ADA_COLS):
            I[j] = c
        index = (I,)
        lists = ta.lists_fixed(I)
    delta = kind.fromf(rng.standard_normal((nb, dim)))
    b = dict(zip(ADA_COLS, pick))
    out = {"name": name, "table": table, "state": state, "delta": delta, "index": index,
           "lists": lists, "planted": sorted(c - 1 for c in ADA_COLS)}
    if plain:
        return out
    st = (lambda c, v: state.__setitem__(c - 1, v))
    delta[b[1]] = pal["zero"]
    st(1, 0)
    delta[b[2]] = _from_bits(tk, rng.integers(1, 1 << (_FMT[tk][3] - 4), dim))
    st(2, 0)
    sgn = np.where(rng.random(dim) < 0.5, -1.0, 1.0)
    sgn[1] = 1.0                                 # -0 - (+0) = -0
    delta[b[4]] = kind.fromf(sgn * 2.0 ** 60)
    st(4, palC["max"])
    table[3, feats] = pal["max_sub"]
    table[3, 1] = pal["-zero"]
    table[3, 2] = pal["-min_sub"]
    delta[b[6], feats], delta[b[7], feats], delta[b[8], feats] = pal["inf"], pal["nan"], pal["-inf"]
    table[8, feats[0]], table[8, feats[-1]] = pal["inf"], pal["-inf"]
    delta[b[15]] = pal["zero"]
    st(15, palC["max_sub"])
    return out


# --- weight gradient -----------------------------------------------------------------------------------

def wgrad_case(dim, kind):
    """weighted_ref.wgrad_case with NaN in one table row and in one bag's gradient (Inf is
    left out: Float32 overflow the Float64 reference does not share has no single right
    answer).  Returns the inputs and the mask of entries that meet a NaN."""
    import weighted_ref as wr

    table, delta, values, colptr, bf16 = wr.wgrad_case(dim, kind)
    pal = palette(kind)["values"]
    row = int(values[len(values) // 2])
    bag = int(np.nonzero(np.diff(colptr) >= 3)[0][5])
    table[row - 1, feats_for(dim)[1]] = pal["nan"]
    delta[bag, dim - 1] = pal["nan"]
    meets = values == row
    meets[colptr[bag] - 1:colptr[bag + 1] - 1] = True
    return table, delta, values, colptr, bf16, meets


# --- quantised lookup ---------------------------------------------------------------------------------

QUANT_CASES = [(8, 128, False), (4, 32, True), (8, 20, False)]  # fused, split header, generic
QUANT_OUTS = ("f32", "f16", "bf16")


def quant_case(bits, dim, P, seed=31):
    """A packed table built directly (no quantiser): 64 ordinary rows and rows whose header
    halves come from the Float16 palette.  The rows take the names forward_bags knows, by the
    role their dequantised values play (v = q * scale + bias in Float32):
      nan         NaN scale and bias (row 1: an out-of-range index must still add +0)
      inf, -inf   +-Inf scale with q != 0 (the last row is `inf`)
      zero_inf    Inf scale with q = 0 (0 * Inf: NaN)
      max, -max   +-65504 scale and bias: finite in Float32, Inf only when rounded to f16
      min_sub ..  +-smallest / largest subnormal scale, bias 0: subnormal only in the f16 output
      min_normal  smallest normal scale
      -zero       q = 0, scale = -smallest subnormal, bias -0: every element -0
      one, -one   scale 0, bias +-1
      nan_bias    scale 1, NaN bias
    Returns levels, scale, bias (float16) and the bags of forward_bags."""
    h = palette("f16")["values"]
    rng = np.random.default_rng([seed, bits, dim, P])
    top = 2 ** bits
    spec = [("nan", h["nan"], h["nan"], None), ("-inf", h["-inf"], h["zero"], 1),
            ("zero_inf", h["inf"], h["one"], 0), ("max", h["max"], h["max"], None),
            ("-max", h["-max"], h["-max"], None), ("min_sub", h["min_sub"], h["zero"], 1),
            ("-min_sub", h["-min_sub"], h["zero"], 1), ("max_sub", h["max_sub"], h["zero"], 1),
            ("-max_sub", h["-max_sub"], h["zero"], 1),
            ("min_normal", h["min_normal"], h["zero"], 1),
            ("-zero", h["-min_sub"], h["-zero"], 0), ("one", h["zero"], h["one"], None),
            ("-one", h["zero"], h["-one"], None), ("nan_bias", h["one"], h["nan"], None),
            ("inf", h["inf"], h["zero"], 1)]
    n = N_ORD + len(spec)
    q = rng.integers(0, top, (n, dim)).astype(np.uint8)
    scale = (rng.random(n) * 0.02 + 0.001).astype(np.float16)
    bias = rng.standard_normal(n).astype(np.float16)
    rows = {}
    for k, (name, s, b, lo) in enumerate(spec):
        r = 1 if name == "nan" else n if name == "inf" else N_ORD + 1 + k
        rows[name] = r
        scale[r - 1], bias[r - 1] = s, b
        if lo == 0:
            q[r - 1] = 0
        elif lo == 1:
            q[r - 1] = rng.integers(1, top, dim)
    assert sorted(rows.values()) == [1] + list(range(N_ORD + 2, n + 1))
    rows["n_ord"] = N_ORD
    values, cp, planted, events = forward_bags(np.full(FWD_B, P), rows, n, seed + P)
    return {"bits": bits, "dim": dim, "q": q, "scale": scale, "bias": bias, "rows": rows,
            "values": values, "colptr": cp, "planted": planted, "events": events}


def quant_pack(case, ld_bytes, split):
    """The packed (R, ld_bytes) uint8 table and the (R, 4) split header array or None."""
    import quant_ref as qr

    bits, dim = case["bits"], case["dim"]
    p = qr.payload_bytes(dim, bits)
    packed = np.full((case["q"].shape[0], ld_bytes), 0xA5, np.uint8)
    packed[:, :p] = qr.pack(case["q"], bits)
    hdr = qr.header_bytes(case["scale"], case["bias"])
    if split:
        return packed, hdr
    packed[:, p:p + 4] = hdr
    return packed, None


def quant_ref(case, out):
    import quant_ref as qr

    with np.errstate(all="ignore"):
        T = qr.dequantize(case["q"], case["scale"], case["bias"])
        P = len(case["values"]) // FWD_B
        return qr.pooled(T, case["values"].reshape(FWD_B, P), out)
