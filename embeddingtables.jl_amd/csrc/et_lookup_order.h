// Item order of the queued pooled lookup's class queues (k_pooled_vec_queued, et_lookup.hip):
// pure index arithmetic, plain C++ with no HIP types, so a host program can include it
// (tests/lookup_order_host.cpp) and the kernel and its test share one definition.
//
// An XCD owns `ntables` entries (one stripe, or one column quarter of half the batch, each;
// "entries" below): [0, nheavy) the FABRIC class, [nheavy,
// ntables) the CACHE class.  Every entry has `sc` chunks; the item (chunk j of entry k) is slot
// j * ntables + k of that XCD (striped_body's numbering, which never changes).  A class queue
// hands out class slots h = 0, 1, 2 ...; the maps below say which item class slot h is.  A class's
// entries are cut into two SEGMENTS, [0, split) and [split, n_class), which run one after the
// other; within a segment the items go either tables fastest (kTablesFastest: chunk 0 of every
// entry, then chunk 1 ..., all the segment's tables in flight together) or table-major
// (kTableMajor: every chunk of the first entry, then the second ..., one table at a time in the
// order the host listed the entries).  For every h < n_class * sc the map is a bijection onto the
// class's items, whatever split and modes say; h beyond that is kNone.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ET_ORDER_FN __host__ __device__ inline
#else
#define ET_ORDER_FN inline
#endif

namespace et_order {

constexpr int kXcds = 8;
constexpr uint32_t kNone = ~0u;
constexpr uint32_t kTablesFastest = 0, kTableMajor = 1;

// One class's order: 16 bytes of the kernel argument.  All zero = the static order (one segment,
// tables fastest).
struct ClassOrder {
    uint8_t split[kXcds];  // per XCD: the class's entries [0, split) are segment 0
    uint8_t major[kXcds];  // per XCD: bit s set = segment s is table-major
};

// Class slot h of a class of `nk` entries starting at entry `base` -> slot j * ntables + k.
ET_ORDER_FN uint32_t class_slot(uint32_t h, uint32_t nk, uint32_t base, uint32_t ntables,
                                uint32_t sc, uint32_t split, uint32_t major0, uint32_t major1) {
    if (h >= nk * sc) return kNone;
    if (split > nk) split = nk;
    uint32_t n = split, first = 0, major = major0;
    if (h >= split * sc) {  // segment 1 (n > 0 in either branch: h is inside the segment)
        h -= split * sc;
        n = nk - split;
        first = split;
        major = major1;
    }
    const uint32_t j = major == kTableMajor ? h % sc : h / n;
    const uint32_t k = major == kTableMajor ? h / sc : h % n;
    return j * ntables + base + first + k;
}

// Class c (0 fabric, 1 cache) of XCD x.
ET_ORDER_FN uint32_t class_slot(const ClassOrder& o, uint32_t x, uint32_t c, uint32_t h,
                                uint32_t nheavy, uint32_t ntables, uint32_t sc) {
    const uint32_t nk = c ? ntables - nheavy : nheavy;
    return class_slot(h, nk, c ? nheavy : 0u, ntables, sc, o.split[x], o.major[x] & 1u,
                      (o.major[x] >> 1) & 1u);
}

// ---- entries.  A whole-row entry is table | stripe << 8: the XCD sums whole rows for the bags of
// that stripe (an eighth of the table's chunks).  A QUARTERED entry is table | half << 8 |
// quarter << 16 | kQuarterFlag: the XCD sums only column quarter `quarter` (one 128-byte line of
// a 512-byte row) for the bags of batch half `half`, so of that table its L2 only ever holds
// every fourth line.  A pooled sum is independent per column: the result does not change.

constexpr uint32_t kQuarterFlag = 1u << 18;

ET_ORDER_FN uint32_t entry_table(uint32_t e) { return e & 0xffu; }
ET_ORDER_FN uint32_t entry_stripe(uint32_t e) { return (e >> 8) & 0xffu; }  // or the half
ET_ORDER_FN uint32_t entry_quarter(uint32_t e) { return (e >> 16) & 3u; }
ET_ORDER_FN bool entry_quartered(uint32_t e) { return (e & kQuarterFlag) != 0; }

// Bags per workgroup round: the scalar-addressed whole-row loop holds two bags per wave; the
// per-lane loop at a quarter of the row holds eight (a group is 8 lanes, not 32).
constexpr int kRowBagsPerRound = 8, kQuarterBagsPerRound = 32;

// Item (entry e, chunk j < sc) of a launch of `nchunks` whole-row chunks of kRowBagsPerRound *
// rounds bags: its chunk number, and the bags [first, first + count) it sums (count 0: an empty
// slot).  A quartered item's chunk is four times as many bags (the same bytes), and the two
// halves' 2 * sc chunks reach the batch because 8 * sc >= nchunks.
struct ItemBags {
    int64_t chunk, first, count;
};
ET_ORDER_FN ItemBags item_bags(uint32_t e, int64_t j, int64_t sc, int64_t nchunks, int64_t rounds,
                               int64_t batch) {
    ItemBags b;
    b.chunk = (int64_t)entry_stripe(e) * sc + j;
    const int64_t per = (entry_quartered(e) ? kQuarterBagsPerRound : kRowBagsPerRound) * rounds;
    b.first = b.chunk * per;
    b.count = 0;
    if (j >= sc || b.first >= batch) return b;
    if (!entry_quartered(e) && b.chunk >= nchunks) return b;
    b.count = batch - b.first < per ? batch - b.first : per;
    return b;
}

// ---- host side.

constexpr int kMaxEntries = 40;  // per XCD (kernel-argument size bound)
constexpr int kMaxTables = 32;   // ET_MAX_TABLES_PER_LAUNCH

// Stripe placement: which stripes XCD x owns.  Heavy tables (above light_bytes) -> stripe x on
// XCD x, listed first; light tables' stripes laid out table after table (alternating large and
// small tables) and cut into kXcds equal runs.  A table of quarter_mask is quartered instead,
// whatever its size: XCD x gets quarter x % 4 of batch half x / 4, one entry per XCD, in the
// fabric class (with the heavy tables, in table order) or, with quarter_cache, at the front of the
// cache class.  *nheavy is the size of the fabric class.  Returns the entries per XCD (= n).
inline int place_stripes(const int64_t* table_bytes, int n, int64_t light_bytes,
                         uint32_t quarter_mask, bool quarter_cache,
                         uint32_t entry[][kMaxEntries], int* nheavy) {
    int heavy[kMaxTables], light[kMaxTables], qcache[kMaxTables];
    int nh = 0, nl = 0, nq = 0;
    auto quartered = [&](int t) { return ((quarter_mask >> t) & 1u) != 0; };
    for (int t = 0; t < n; ++t)
        if (quartered(t) && quarter_cache) qcache[nq++] = t;
        else if (quartered(t) || table_bytes[t] > light_bytes) heavy[nh++] = t;
        else light[nl++] = t;
    auto quarter_entry = [](int t, int x) {
        return (uint32_t)t | ((uint32_t)(x / 4) << 8) | ((uint32_t)(x % 4) << 16) | kQuarterFlag;
    };
    // light tables by size, then interleave large / small
    for (int a = 0; a < nl; ++a)
        for (int b = a + 1; b < nl; ++b)
            if (table_bytes[light[b]] > table_bytes[light[a]]) {
                int tmp = light[a];
                light[a] = light[b];
                light[b] = tmp;
            }
    int order[kMaxTables];
    for (int i = 0, lo = 0, hi = nl - 1; i < nl; ++i) order[i] = (i & 1) ? light[hi--] : light[lo++];
    int cnt[kXcds] = {0};
    for (int x = 0; x < kXcds; ++x) {
        for (int h = 0; h < nh; ++h)
            entry[x][cnt[x]++] = quartered(heavy[h]) ? quarter_entry(heavy[h], x)
                                                     : (uint32_t)heavy[h] | ((uint32_t)x << 8);
        for (int h = 0; h < nq; ++h) entry[x][cnt[x]++] = quarter_entry(qcache[h], x);
    }
    // linear list of light stripes (order[i], st), st < kXcds; XCD x takes [x*nl, (x+1)*nl)
    for (int q = 0; q < nl * kXcds; ++q) {
        const int x = q / (nl > 0 ? nl : 1);
        entry[x][cnt[x]++] = (uint32_t)order[q / kXcds] | ((uint32_t)(q % kXcds) << 8);
    }
    *nheavy = nh;
    return cnt[0];
}

// No table quartered.
inline int place_stripes(const int64_t* table_bytes, int n, int64_t light_bytes,
                         uint32_t entry[][kMaxEntries], int* nheavy) {
    return place_stripes(table_bytes, n, light_bytes, 0u, false, entry, nheavy);
}
// The order of an XCD's entries within a class (placement never changes: each function below
// permutes e[0, n) in place).

// Stable: entries for which first(e) holds move to the front.  Returns how many.
template <typename F>
inline int stable_front(uint32_t* e, int n, F first) {
    uint32_t tmp[256];
    int a = 0, b = 0;
    for (int i = 0; i < n; ++i)
        if (first(e[i])) e[a++] = e[i];
        else tmp[b++] = e[i];
    for (int i = 0; i < b; ++i) e[a + i] = tmp[i];
    return a;
}

// Rotate e[0, n) left by r.
inline void rotate_left(uint32_t* e, int n, int r) {
    if (n <= 1) return;
    uint32_t tmp[256];
    for (int i = 0; i < n; ++i) tmp[i] = e[(i + r) % n];
    for (int i = 0; i < n; ++i) e[i] = tmp[i];
}

// Cache class, table-major: the entries by table size, largest first (stable insertion sort, so
// a table's stripes stay together in their order).
inline void largest_first(uint32_t* e, int n, const int64_t* table_bytes) {
    for (int i = 1; i < n; ++i) {
        const uint32_t v = e[i];
        int k = i;
        for (; k > 0 && table_bytes[entry_table(e[k - 1])] < table_bytes[entry_table(v)]; --k)
            e[k] = e[k - 1];
        e[k] = v;
    }
}

// L2 footprint of an XCD's cache class: the bytes of the distinct tables among e[0, n).
inline int64_t class_footprint(const uint32_t* e, int n, const int64_t* table_bytes) {
    uint32_t seen = 0;
    int64_t sum = 0;
    for (int i = 0; i < n; ++i) {
        const uint32_t t = entry_table(e[i]);
        if (!((seen >> t) & 1u)) sum += table_bytes[t];
        seen |= 1u << t;
    }
    return sum;
}

// Fabric class in two phases: the non-temporal tables (nt_mask; they never allocate in L2) and
// the allocating ones.  nt_first puts the non-temporal phase first.  The allocating group is
// rotated left by `rot` (table-major: each XCD starts on another table).  Returns the split:
// the number of entries in the first phase.
inline int two_phases(uint32_t* e, int n, uint32_t nt_mask, bool nt_first, int rot) {
    const int nnt =
        stable_front(e, n, [&](uint32_t v) { return ((nt_mask >> entry_table(v)) & 1u) != 0; });
    const int nal = n - nnt;
    if (nal > 0) rotate_left(e + nnt, nal, rot % nal);
    if (nt_first) return nnt;
    rotate_left(e, n, nnt);  // allocating group to the front, both groups keep their order
    return nal;
}

// The policies (DESIGN section 4 "L2 order").  All zero = the static order; the library's choice
// is LookupTuning::order (et_lookup.hip).
struct Policy {
    int cache_major = 0;  // (a) cache class table-major, each XCD's largest light table first
    // fabric class: 0 tables fastest; 1 (b) two phases, tables fastest within each; 2 (b) + (c)
    // two phases, the allocating one table-major and rotated by XCD; 3 the whole class
    // table-major, rotated by XCD
    int fab = 0;
    // (b): an XCD whose cache class holds more than this runs its non-temporal phase first (while
    // its big light table runs under (a)), the others run it last
    int64_t phase_bytes = 1 << 20;
};

// Orders XCD x's entries e[0, ntables) within their classes and fills x's part of ord[0]
// (fabric) and ord[1] (cache).
inline void order_xcd(uint32_t* e, int x, int ntables, int nheavy, const int64_t* table_bytes,
                      uint32_t nt_mask, const Policy& p, ClassOrder ord[2]) {
    uint32_t* ce = e + nheavy;
    const int nc = ntables - nheavy;
    ord[0].split[x] = ord[1].split[x] = 0;
    ord[0].major[x] = ord[1].major[x] = 0;
    if (p.cache_major) {
        largest_first(ce, nc, table_bytes);
        ord[1].major[x] = 3;
    }
    if (p.fab == 1 || p.fab == 2) {
        const bool nt_first = class_footprint(ce, nc, table_bytes) > p.phase_bytes;
        ord[0].split[x] = (uint8_t)two_phases(e, nheavy, nt_mask, nt_first, p.fab == 2 ? x : 0);
        if (p.fab == 2) ord[0].major[x] = nt_first ? 2 : 1;  // the allocating segment
    } else if (p.fab == 3) {
        rotate_left(e, nheavy, nheavy > 0 ? x % nheavy : 0);
        ord[0].major[x] = 3;
    }
}

}  // namespace et_order
