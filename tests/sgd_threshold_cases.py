"""Case builders and host predicates shared by tests/test_gpu_sgd_thresholds.py and
tests/test_sgd_threshold_cases_host.py.  It holds no tests and no fixtures, and nothing here
touches a device: every builder returns numpy arrays and plain Python values.

The default (exact) sparse SGD sums a column of more than CHUNK occurrences as a serial chain,
planned by one of three planners of embeddingtables.jl_amd/csrc/et_update.hip: the early chains
(EC, `ec_table`), the early hot columns (EH, `eh_table` and `k_eh_pick`) and the regular plan
(`k_chain_*`, tiles of TILE occurrences with a HALO).  The builders here shape index matrices

* whose runs (r occurrences of one column inside one bag) sit at chosen places of the regular
  plan's tiles (``halo_case``, ``tiny_pool_case``, ``long_run_case``), and
* that stand on both sides of every threshold between the planners (``pool_pair_case`` ...
  ``crowded_case``) and of the split mode's hot pass (``hot_pass_case``),

and the predicates restate what the kernels compute from an index matrix: a column's run list,
the sample counts of `k_eh_pick`, its candidate test and the occupancy of its LDS hash.  The
constants are mirrored with their source lines in tests/test_gpu_sgd_thresholds.py.

The small cases are built once and shared (``lru_cache``): a test copies what it updates in
place.  The cases of 2^20 bags are not cached."""
import functools

import numpy as np

CHUNK = 256              # ET_SGD_CHUNK: a longer column is a chain in the exact mode
TILE = 4096              # kChainTile
HALO = 64                # kChainHalo
EC_MAX_ROWS = 128        # kEcMaxRows
EC_MAX_POOL = 255        # kEcMaxPool
EC_MAX_BATCH = 1 << 20   # kEcMaxBatch
EH_SAMPLE_BAGS = 1024    # kEhSampleBags
EH_MIN_OCC = 32768       # kEhMinOcc
EH_K = 16                # kEhK
EH_QUALIFY = 512         # qk / qc of k_eh_pick
EH_HASH = 4096           # kEhHash
EH_PROBES = 16           # kEhProbes
HOT_MAX_POOL = 32        # kHotMaxPool
DIM = 16


# --- host predicates ---------------------------------------------------------------------------

def as_matrix(I):
    I = np.asarray(I)
    return I.reshape(-1, 1) if I.ndim == 1 else I


def column_counts(I, R):
    """Occurrences of every column (1-based; index 0 of the result unused)."""
    return np.bincount(np.asarray(I).reshape(-1), minlength=R + 1)


def runs_of(I, col):
    """(heads, lengths) of column `col`'s runs: its occurrence list is bag-major (the sort is
    stable), so bag b holds the r_b = lengths[k] consecutive positions from heads[k] =
    r_0 + ... + r_(b-1) on."""
    r = (as_matrix(I) == col).sum(axis=1)
    r = r[r > 0]
    return np.cumsum(r) - r, r


def tiles_without_head(heads, total):
    """Tiles of a column of `total` occurrences in which no run starts."""
    have = set((np.asarray(heads) // TILE).tolist())
    return [t for t in range(-(-total // TILE)) if t not in have]


def sample_counts(I, R):
    """What k_eh_pick counts when its hash drops nothing: the columns of the first
    min(B, EH_SAMPLE_BAGS) bags."""
    I = as_matrix(I)
    return column_counts(I[:min(len(I), EH_SAMPLE_BAGS)], R)


def eh_qualifies(count, B):
    """k_eh_pick's candidate test: count * batch >= kEhMinOcc * sampled bags."""
    return count * B >= EH_MIN_OCC * min(B, EH_SAMPLE_BAGS)


def eh_qualifying(I, R):
    """The columns (1-based, ascending) that pass the candidate test on exact sample counts."""
    I = as_matrix(I)
    c = sample_counts(I, R)
    return np.flatnonzero(eh_qualifies(c, len(I)) & (np.arange(R + 1) > 0))


def eh_pick(I, R):
    """The candidates k_eh_pick keeps when nothing is dropped and at most EH_QUALIFY columns
    qualify: the EH_K most frequent in the sample, ties to the smaller column."""
    q = eh_qualifying(I, R)
    assert len(q) <= EH_QUALIFY
    c = sample_counts(I, R)[q]
    return np.sort(q[np.lexsort((q, -c))][:EH_K])


def ec_table(R, P, B):
    return 0 < R <= EC_MAX_ROWS and 0 < P <= EC_MAX_POOL and 0 < B <= EC_MAX_BATCH


def eh_table(R, P, B):
    return R > EC_MAX_ROWS and 0 < P <= EC_MAX_POOL and 0 < B <= EC_MAX_BATCH


def hash_longest_cluster(I, R):
    """The longest stretch of occupied slots of k_eh_pick's hash once every distinct sampled
    column has a slot (linear probing from ((c - 1) * 2654435761 mod 2^32) >> 20; which slots
    end up occupied does not depend on the arrival order).  At most EH_PROBES: no arrival
    order drops an occurrence.  EH_HASH: more columns than slots."""
    cols = np.flatnonzero(sample_counts(I, R)[1:])  # 0-based, as the kernel hashes them
    if len(cols) >= EH_HASH:
        return EH_HASH
    used = np.zeros(EH_HASH, bool)
    product = cols.astype(np.uint64) * np.uint64(2654435761)
    for h in ((product & np.uint64(0xffffffff)) >> np.uint64(20)).tolist():
        while used[h]:
            h = (h + 1) % EH_HASH
        used[h] = True
    start = int(np.flatnonzero(~used)[0])
    best = run = 0
    for u in np.roll(used, -start):
        run = run + 1 if u else 0
        best = max(best, run)
    return best


# --- draws -------------------------------------------------------------------------------------

def zipf_draw(rng, R, shape):
    """1-based indices with P(rank k) proportional to k^-1.05 over a random ranking of R
    columns (every column of a 3-row table gets a share: 0.54, 0.26, 0.17)."""
    p = np.arange(1, R + 1, dtype=np.float64) ** -1.05
    x = rng.choice(R, shape, p=p / p.sum())
    return (rng.permutation(R)[x] + 1).astype(np.int64)


def normal32(rng, shape):
    return rng.standard_normal(shape, dtype=np.float32)


def blocks_with_counts(rng, nblocks, slots, counted, others):
    """(nblocks, slots) int64: every row holds column c exactly n times for (c, n) in
    `counted` and uniform draws of `others` elsewhere, shuffled within the row."""
    fixed = np.concatenate([np.full(n, c, np.int32) for c, n in counted])
    m = np.empty((nblocks, slots), np.int32)
    m[:, :len(fixed)] = fixed
    m[:, len(fixed):] = rng.choice(np.asarray(others, np.int32), (nblocks, slots - len(fixed)))
    return rng.permuted(m, axis=1).astype(np.int64)


# --- A1. halo and tile alignment ---------------------------------------------------------------

HALO_H, HALO_G = 7, 150  # the column of placed runs; the column of runs inside the halo


def halo_h_runs():
    """H's runs r_b in bag order.  Heads and ends follow from the cumulative sums: the eight
    short lengths, a run that ends on tile 0's last slot, a run of 100 on tile 1's first,
    heads on the last slots of tiles 1, 2 and 3 with 64, 65 and 66 occurrences, a run of 100
    with 6 occurrences before the end of tile 4, and a tail."""
    runs = [1, 15, 16, 17, 63, 64, 65, 66]

    def fill(target):  # runs of 100 (the last one shorter) up to position `target`
        while sum(runs) < target:
            runs.append(min(100, target - sum(runs)))

    fill(TILE)
    runs.append(100)
    for k, r in ((2, 64), (3, 65), (4, 66)):
        fill(k * TILE - 1)
        runs.append(r)
    fill(5 * TILE - 6)
    runs.append(100)
    return runs + [40, 3]


@functools.lru_cache(maxsize=None)
def halo_case():
    """200 rows, 300 bags of 100: column H's runs of ``halo_h_runs`` in randomly chosen bags,
    column G with runs of 17..40 in the bags H leaves at least 40 slots of, the rest uniform
    over the other columns; every bag shuffled."""
    rng = np.random.default_rng(0xA1)
    R, B, P = 200, 300, 100
    runs = halo_h_runs()
    rh = np.zeros(B, np.int64)
    rh[np.sort(rng.choice(B, len(runs), replace=False))] = runs
    rg = np.zeros(B, np.int64)
    room = np.flatnonzero(rh <= 60)
    rg[room] = 17 + np.arange(len(room)) % 24
    others = np.setdiff1d(np.arange(1, R + 1), [HALO_H, HALO_G])
    I = np.empty((B, P), np.int64)
    for b in range(B):
        row = np.concatenate([np.full(rh[b], HALO_H), np.full(rg[b], HALO_G),
                              rng.choice(others, P - rh[b] - rg[b])])
        I[b] = rng.permutation(row)
    return {"R": R, "B": B, "P": P, "I": I, "H": HALO_H, "G": HALO_G,
            "table": normal32(rng, (R, DIM)), "delta": normal32(rng, (B, DIM))}


# --- A2. pool above 255 on a tiny table --------------------------------------------------------

@functools.lru_cache(maxsize=None)
def tiny_pool_case(P):
    """3 rows, 64 bags of P = 256 or 300 Zipf indices; bag 17 is the most frequent column
    throughout (its other runs are about 0.54 * P long: beyond the halo as well)."""
    rng = np.random.default_rng([0xA2, P])
    R, B = 3, 64
    I = zipf_draw(rng, R, (B, P))
    top = int(np.argmax(column_counts(I, R)))
    I[17] = top
    return {"R": R, "B": B, "P": P, "I": I, "full_bag": 17, "full_col": top,
            "table": normal32(rng, (R, DIM)), "delta": normal32(rng, (B, DIM))}


# --- A3. a run longer than a tile --------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def long_run_case():
    """3 rows, 12 bags of 5,000.  Column 1: 4,000 occurrences in bag 0, all 5,000 of bag 1
    (positions 4,000..8,999 of its list: tile 1 holds no head) and 4,000 of bag 2.  Column 3,
    the last key of the sorted list, ends it with a run of 4,500 in the last bag."""
    rng = np.random.default_rng(0xA3)
    R, B, P = 3, 12, 5000
    I = zipf_draw(rng, R, (B, P))
    for b in (0, 2):
        I[b] = rng.permutation(np.concatenate([np.full(4000, 1), rng.choice([2, 3], 1000)]))
    I[1] = 1
    I[B - 1] = rng.permutation(np.concatenate([np.full(4500, 3), rng.choice([1, 2], 500)]))
    return {"R": R, "B": B, "P": P, "I": I,
            "table": normal32(rng, (R, DIM)), "delta": normal32(rng, (B, DIM))}


# --- A6. occurrence offsets --------------------------------------------------------------------

OFFSET_K = 3  # prepended gradient columns


@functools.lru_cache(maxsize=None)
def offsets_case():
    """A 5-row, pool-7 table of 129 bags, then the tables of halo_case, tiny_pool_case(300) and
    long_run_case: the occurrence offsets of tables 2 to 4 are 903, 30,903 and 50,103.  One
    gradient of 300 rows and 3 + 4 * 16 columns; table t reads its first B_t rows."""
    rng = np.random.default_rng(0xA6)
    first = {"R": 5, "B": 129, "P": 7, "I": zipf_draw(rng, 5, (129, 7)),
             "table": normal32(rng, (5, DIM))}
    tabs = [first, halo_case(), tiny_pool_case(300), long_run_case()]
    occ = np.cumsum([0] + [t["B"] * t["P"] for t in tabs])
    return {"tables": tabs, "occ_off": occ[:-1].tolist(),
            "offs": [OFFSET_K + DIM * t for t in range(len(tabs))],
            "delta": normal32(rng, (300, OFFSET_K + DIM * len(tabs)))}


# --- B1. pool 255 | 256 ------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def pool_pair_case():
    """300 bags of 256 for a 3-row and a 1,000-row table; the pool-255 side is the first 255
    columns of the same draw.  Bag 41 of the 3-row table is column 3 throughout (a byte
    counter of 255); column 500 of the large table has a 45 % share, column 77 a 3 % one."""
    rng = np.random.default_rng(0xB1)
    B, P = 300, 256
    small = zipf_draw(rng, 3, (B, P))
    small[41] = 3
    u = rng.random((B, P))
    large = np.where(u < 0.45, 500, np.where(u < 0.48, 77, rng.integers(1, 1001, (B, P))))
    return {"B": B, "P": P, "I": [small, large.astype(np.int64)], "rows": [3, 1000],
            "hot": 500, "tables": [normal32(rng, (3, DIM)), normal32(rng, (1000, DIM))],
            "delta": normal32(rng, (B, 2 * DIM))}


# --- B2. batch 2^20 | 2^20 + 1 -----------------------------------------------------------------

BATCH_X, BATCH_Y, BATCH_W = 100, 200, 300


def batch_pair_case():
    """2^20 + 1 bags of one index for a 3-row (Zipf) and a 1,000-row table; the 2^20 side is the
    first 2^20 bags.  Every 1,024 bags of the large table hold column X 32 times, Y 31 times
    and W 60 times, the rest uniform over the other columns."""
    rng = np.random.default_rng(0xB2)
    B = EC_MAX_BATCH + 1
    others = np.setdiff1d(np.arange(1, 1001), [BATCH_X, BATCH_Y, BATCH_W])
    large = blocks_with_counts(rng, B // 1024 + 1, 1024,
                               [(BATCH_X, 32), (BATCH_Y, 31), (BATCH_W, 60)], others)
    return {"B": B, "I": [zipf_draw(rng, 3, B), large.reshape(-1)[:B].copy()], "rows": [3, 1000],
            "tables": [normal32(rng, (3, DIM)), normal32(rng, (1000, DIM))],
            "delta": normal32(rng, (B, 2 * DIM))}


# --- B3. the sample is the whole batch ---------------------------------------------------------

@functools.lru_cache(maxsize=None)
def sample_case():
    """1,025 bags of 40 for two 1,000-row tables (a column's share is of one table's slots):
    column 321 of the first has an 85 % share, column 654 of the second a 70 % one.  The
    1,023- and 1,024-bag sides are the first bags of the same draw."""
    rng = np.random.default_rng(0xB3)
    B, P = 1025, 40
    I = [np.where(rng.random((B, P)) < share, col, rng.integers(1, 1001, (B, P))).astype(np.int64)
         for share, col in ((0.85, 321), (0.70, 654))]
    return {"B": B, "P": P, "I": I, "rows": [1000, 1000], "hot": [321, 654],
            "tables": [normal32(rng, (1000, DIM)), normal32(rng, (1000, DIM))],
            "delta": normal32(rng, (B, 2 * DIM))}


# --- B4. a candidate that is not a chain -------------------------------------------------------

NAC_X, NAC_Y, NAC_Z = 10, 20, 30


@functools.lru_cache(maxsize=None)
def not_a_chain_case():
    """131,072 bags of one index, 1,000 rows.  X 256 times and Y 257 times, all in the first
    1,024 bags; Z 40,000 times, none of them there; the rest uniform over the other columns."""
    rng = np.random.default_rng(0xB4)
    B, R = 131072, 1000
    others = np.setdiff1d(np.arange(1, R + 1), [NAC_X, NAC_Y, NAC_Z])
    head = blocks_with_counts(rng, 1, 1024, [(NAC_X, 256), (NAC_Y, 257)], others)
    rest = blocks_with_counts(rng, 1, B - 1024, [(NAC_Z, 40000)], others)
    return {"B": B, "R": R, "P": 1, "I": np.concatenate([head[0], rest[0]]),
            "table": normal32(rng, (R, DIM)), "delta": normal32(rng, (B, DIM))}


# --- B5. more candidates than slots, with ties -------------------------------------------------

TIE_COLS = tuple(40 + 47 * i for i in range(20))
TIE_POOL = 8     # 20 tied columns at or above the threshold of 256 need 5,120 sampled slots
TIE_COUNT = 300  # of every tied column in every 1,024 bags


@functools.lru_cache(maxsize=None)
def tie_case():
    """131,072 bags of 8, 1,000 rows: every 1,024 bags hold each of 20 columns exactly 300
    times (above the candidate threshold of 256), the rest uniform over the other columns."""
    rng = np.random.default_rng(0xB5)
    B, R, P = 131072, 1000, TIE_POOL
    others = np.setdiff1d(np.arange(1, R + 1), TIE_COLS)
    I = blocks_with_counts(rng, B // 1024, 1024 * P, [(c, TIE_COUNT) for c in TIE_COLS], others)
    return {"B": B, "R": R, "P": P, "I": I.reshape(B, P),
            "table": normal32(rng, (R, DIM)), "delta": normal32(rng, (B, DIM))}


# --- B6. more than 512 qualifying columns ------------------------------------------------------

QUALIFY_COLS = 600


def qualify_case():
    """2^20 bags of 20, 700 rows: every 1,024 bags hold each of the first 600 columns exactly
    33 times (19,800 of 20,480 slots), the rest uniform over the last 100.  No gradient: the
    GPU test fills it on the device."""
    rng = np.random.default_rng(0xB6)
    B, R, P = 1 << 20, 700, 20
    I = blocks_with_counts(rng, B // 1024, 1024 * P,
                           [(c, 33) for c in range(1, QUALIFY_COLS + 1)],
                           np.arange(QUALIFY_COLS + 1, R + 1))
    return {"B": B, "R": R, "P": P, "I": I.reshape(B, P), "table": normal32(rng, (R, DIM))}


# --- B7. crowded sample hash -------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def crowded_case():
    """4,096 bags of 20, 100,000 rows: column 31,337 has a 45 % share, the rest is uniform."""
    rng = np.random.default_rng(0xB7)
    B, R, P = 4096, 100000, 20
    I = np.where(rng.random((B, P)) < 0.45, 31337, rng.integers(1, R + 1, (B, P)))
    return {"B": B, "R": R, "P": P, "I": I.astype(np.int64), "hot": 31337,
            "table": normal32(rng, (R, DIM)), "delta": normal32(rng, (B, DIM))}


# --- C. split-mode hot pass, pool 32 | 33 ------------------------------------------------------

@functools.lru_cache(maxsize=None)
def hot_pass_case():
    """1,500 bags of 33 Zipf indices into 300 rows, a dim-128 table and gradient; the pool-32
    side is the first 32 columns of the draw, the dim-124 table the first 124 features."""
    rng = np.random.default_rng(0xC)
    B, R, P, D = 1500, 300, HOT_MAX_POOL + 1, 128
    return {"B": B, "R": R, "P": P, "D": D, "I": zipf_draw(rng, R, (B, P)),
            "table": normal32(rng, (R, D)), "delta": normal32(rng, (B, D))}
