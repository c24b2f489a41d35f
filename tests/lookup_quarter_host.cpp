// Stand-alone check of the quartered entries of csrc/et_lookup_order.h (built and run by
// tests/test_lookup_quarter_host.py with -fsanitize=address,undefined).  For every ntables 2..32,
// every number 0..ntables of quartered tables among them (in the fabric class and in the cache
// class), stripe_chunks in {1, 2, 3, 65, 128}, rounds in {1, 8} and batch sizes around every
// boundary:
//   * every XCD has exactly ntables entries, one for each quartered and each heavy table (its
//     run of the light tables' stripes may hold several stripes of one table, as before);
//   * the eight (quarter, half) pairs of a quartered table are each owned by exactly one XCD, and
//     XCD x owns quarter x % 4 of half x / 4;
//   * over all XCDs and items, every (bag < batch, quarter) of a quartered table and every
//     (bag < batch, whole row) of the other tables is covered exactly once, and no item reaches
//     beyond the batch;
//   * the class order (order_xcd) only permutes the entries within their class;
//   * with nothing quartered, the entries equal those of the placement before quartering existed
//     (restated below), through the old and the new signature.
#include <stdio.h>
#include <string.h>

#include <atomic>
#include <thread>
#include <vector>

#include "et_lookup_order.h"

using namespace et_order;

static std::atomic<int> g_fail{0};
static std::atomic<long> g_cases{0};
#define CHECK(cond, ...)                    \
    do {                                    \
        if (!(cond)) {                      \
            if (g_fail++ < 20) {            \
                printf("FAIL %s: ", #cond); \
                printf(__VA_ARGS__);        \
                printf("\n");               \
            }                               \
        }                                   \
    } while (0)

static const int kSc[] = {1, 2, 3, 65, 128};
static const int kRounds[] = {1, 8};
static const int64_t kLight = 4 << 20;

// The placement as it was before quartered entries: heavy tables' stripe x on XCD x, listed
// first; the light tables' stripes by size, large and small alternating, cut into eight runs.
static int place_before(const int64_t* bytes, int n, uint32_t entry[][kMaxEntries], int* nheavy) {
    std::vector<int> heavy, light;
    for (int t = 0; t < n; ++t) (bytes[t] > kLight ? heavy : light).push_back(t);
    const int nl = (int)light.size();
    for (int a = 0; a < nl; ++a)
        for (int b = a + 1; b < nl; ++b)
            if (bytes[light[b]] > bytes[light[a]]) std::swap(light[a], light[b]);
    std::vector<int> order(nl);
    for (int i = 0, lo = 0, hi = nl - 1; i < nl; ++i) order[i] = (i & 1) ? light[hi--] : light[lo++];
    int cnt[kXcds] = {0};
    for (int x = 0; x < kXcds; ++x)
        for (int t : heavy) entry[x][cnt[x]++] = (uint32_t)t | ((uint32_t)x << 8);
    for (int q = 0; q < nl * kXcds; ++q) {
        const int x = q / nl;
        entry[x][cnt[x]++] = (uint32_t)order[q / kXcds] | ((uint32_t)(q % kXcds) << 8);
    }
    *nheavy = (int)heavy.size();
    return cnt[0];
}

// Sizes: every third table heavy (some above 16 MiB), the others light; `nq` tables, spread over
// the table ids, are the quartered ones (their sizes do not matter to the placement: the mask
// decides, so light and heavy ones are both among them).
static void make_tables(int n, int nq, int64_t* bytes, uint32_t* qmask) {
    *qmask = 0;
    for (int t = 0; t < n; ++t) {
        bytes[t] = t % 3 == 1 ? kLight + 512ll * (1 + (int64_t)((t * 2654435761u) % 60000u))
                              : 512ll * (3 + (int64_t)((t * 2654435761u) % 8000u));
        if ((t + 1) * nq / n > t * nq / n) *qmask |= 1u << t;
    }
}

// The coverage of one launch: hits[t][q][chunk] over every XCD's items.
static void check_coverage(const uint32_t entry[][kMaxEntries], int n, uint32_t qmask, int sc,
                           int rounds, int64_t batch, std::vector<int>& hits) {
    const int64_t nchunks = (batch + kRowBagsPerRound * rounds - 1) / (kRowBagsPerRound * rounds);
    const int maxc = kXcds * sc;  // chunk numbers per (table, quarter): 8 stripes or 2 halves
    hits.assign((size_t)n * 4 * maxc, 0);
    for (int x = 0; x < kXcds; ++x)
        for (int k = 0; k < n; ++k) {
            const uint32_t e = entry[x][k];
            const int t = (int)entry_table(e);
            const bool qd = entry_quartered(e);
            const int64_t per = (qd ? kQuarterBagsPerRound : kRowBagsPerRound) * rounds;
            for (int j = 0; j < sc; ++j) {
                const ItemBags b = item_bags(e, j, sc, nchunks, rounds, batch);
                CHECK(b.chunk == (int64_t)entry_stripe(e) * sc + j && b.chunk < maxc, "chunk");
                CHECK(b.first == b.chunk * per, "first bag: e %08x j %d", e, j);
                if (b.first >= batch) {
                    CHECK(b.count == 0, "item beyond the batch runs: e %08x j %d batch %ld", e, j,
                          (long)batch);
                    continue;
                }
                const int64_t want = batch - b.first < per ? batch - b.first : per;
                CHECK(b.count == want, "bags of item: e %08x j %d batch %ld: %ld, expected %ld", e, j,
                      (long)batch, (long)b.count, (long)want);
                if (b.chunk < maxc) ++hits[((size_t)t * 4 + (qd ? entry_quarter(e) : 0)) * maxc + b.chunk];
            }
            // the kernel's early return for the slots past the entry's chunks
            CHECK(item_bags(e, sc, sc, nchunks, rounds, batch).count == 0, "j == sc runs");
        }
    for (int t = 0; t < n; ++t) {
        const bool qd = (qmask >> t) & 1u;
        const int64_t per = (qd ? kQuarterBagsPerRound : kRowBagsPerRound) * rounds;
        for (int q = 0; q < 4; ++q)
            for (int c = 0; c < maxc; ++c) {
                const int want = (qd || q == 0) && (int64_t)c * per < batch ? 1 : 0;
                const int got = hits[((size_t)t * 4 + q) * maxc + c];
                CHECK(got == want,
                      "n %d sc %d rounds %d batch %ld table %d (%s) quarter %d chunk %d covered %d times",
                      n, sc, rounds, (long)batch, t, qd ? "quartered" : "whole", q, c, got);
            }
    }
}

static void run_tables(int n) {
    long cases = 0;
    std::vector<int> hits;
    for (int nq = 0; nq <= n; ++nq)
        for (int qcache = 0; qcache < 2; ++qcache) {
            int64_t bytes[kMaxTables], foot[kMaxTables];
            uint32_t qmask;
            make_tables(n, nq, bytes, &qmask);
            uint32_t entry[kXcds][kMaxEntries];
            int nh = -1;
            const int nent = place_stripes(bytes, n, kLight, qmask, qcache != 0, entry, &nh);
            CHECK(nent == n, "entries per XCD: n %d nq %d -> %d", n, nq, nent);

            // one entry per table on every XCD; the (quarter, half) pairs and the stripes once each
            int owner[kMaxTables][kXcds];  // [t][pair or stripe] -> how many XCDs own it
            memset(owner, 0, sizeof(owner));
            int want_nh = 0;
            for (int t = 0; t < n; ++t) {
                const bool qd = (qmask >> t) & 1u;
                if (qd ? !qcache : bytes[t] > kLight) ++want_nh;
            }
            CHECK(nh == want_nh, "fabric class size: n %d nq %d qcache %d: %d, expected %d", n, nq,
                  qcache, nh, want_nh);
            for (int x = 0; x < kXcds; ++x) {
                uint32_t tables = 0;
                for (int k = 0; k < nent; ++k) {
                    const uint32_t e = entry[x][k], t = entry_table(e);
                    CHECK(t < (uint32_t)n, "entry %08x", e);
                    if (t >= (uint32_t)n) continue;
                    const bool qd = (qmask >> t) & 1u;
                    // (an XCD may hold several stripes of one light table: its run of the list)
                    if (qd || bytes[t] > kLight) {
                        CHECK(!((tables >> t) & 1u), "XCD %d lists table %u twice", x, t);
                        tables |= 1u << t;
                    }
                    CHECK(entry_quartered(e) == qd, "flag of entry %08x", e);
                    CHECK((e >> 19) == 0, "bits above the flag: %08x", e);
                    const bool fabric = qd ? !qcache : bytes[t] > kLight;
                    CHECK(fabric == (k < nh), "class boundary: x %d k %d e %08x", x, k, e);
                    if (qd) {
                        CHECK(entry_quarter(e) == (uint32_t)(x % 4) && entry_stripe(e) == (uint32_t)(x / 4),
                              "XCD %d owns quarter %u of half %u", x, entry_quarter(e), entry_stripe(e));
                        if (entry_stripe(e) < 2) ++owner[t][entry_stripe(e) * 4 + entry_quarter(e)];
                    } else {
                        CHECK(entry_stripe(e) < (uint32_t)kXcds && ((e >> 16) & 7u) == 0, "entry %08x", e);
                        if (entry_stripe(e) < (uint32_t)kXcds) ++owner[t][entry_stripe(e)];
                        if (fabric) CHECK(entry_stripe(e) == (uint32_t)x, "heavy stripe: x %d e %08x", x, e);
                    }
                }
                uint32_t once = qmask;  // the quartered and the heavy tables: one entry on every XCD
                for (int t = 0; t < n; ++t)
                    if (bytes[t] > kLight) once |= 1u << t;
                CHECK(tables == once, "XCD %d misses a table: %08x of %08x", x, tables, once);
            }
            for (int t = 0; t < n; ++t)
                for (int i = 0; i < kXcds; ++i)
                    CHECK(owner[t][i] == 1, "n %d nq %d table %d part %d owned %d times", n, nq, t, i,
                          owner[t][i]);

            if (nq == 0) {  // nothing quartered: today's entries, through either signature
                uint32_t before[kXcds][kMaxEntries], old_sig[kXcds][kMaxEntries];
                int nhb = -1, nho = -1;
                const int nb = place_before(bytes, n, before, &nhb);
                const int no = place_stripes(bytes, n, kLight, old_sig, &nho);
                CHECK(nb == nent && nhb == nh && no == nent && nho == nh, "counts without quarters");
                for (int x = 0; x < kXcds; ++x)
                    for (int k = 0; k < nent; ++k)
                        CHECK(before[x][k] == entry[x][k] && old_sig[x][k] == entry[x][k],
                              "n %d x %d k %d: %08x, before %08x, old signature %08x", n, x, k,
                              entry[x][k], before[x][k], old_sig[x][k]);
            }

            // the shipped class order permutes within the classes; the cache class goes by what an
            // XCD's L2 holds of a table (a quarter of a quartered one), largest first
            for (int t = 0; t < n; ++t) foot[t] = ((qmask >> t) & 1u) ? bytes[t] / 4 : bytes[t];
            uint32_t ordered[kXcds][kMaxEntries];
            memcpy(ordered, entry, sizeof(ordered));
            ClassOrder ord[2];
            Policy p;
            p.cache_major = 1;
            p.fab = 3;
            for (int x = 0; x < kXcds; ++x) {
                order_xcd(ordered[x], x, nent, nh, foot, 0u, p, ord);
                for (int c = 0; c < 2; ++c) {
                    const int lo = c ? nh : 0, hi = c ? nent : nh;
                    for (int k = lo; k < hi; ++k) {
                        int found = 0;
                        for (int m = lo; m < hi; ++m) found += ordered[x][m] == entry[x][k];
                        CHECK(found == 1, "order moved entry %08x out of its class", entry[x][k]);
                    }
                }
                for (int k = nh + 1; k < nent; ++k)
                    CHECK(foot[entry_table(ordered[x][k - 1])] >= foot[entry_table(ordered[x][k])],
                          "cache order by footprint: x %d k %d", x, k);
            }

            for (int sc : kSc)
                for (int rounds : kRounds) {
                    const int64_t half = (int64_t)kQuarterBagsPerRound * rounds * sc, full = 2 * half;
                    const int64_t r32 = (int64_t)kQuarterBagsPerRound * rounds;
                    const int64_t batches[] = {1, 31, 32, 33, r32 - 1, r32, r32 + 1, half - 1,
                                               half, half + 1, full - 1, full};
                    int64_t done[12];
                    int nd = 0;
                    for (int64_t batch : batches) {
                        if (batch < 1 || batch > full) continue;
                        bool dup = false;
                        for (int i = 0; i < nd; ++i) dup |= done[i] == batch;
                        if (dup) continue;
                        done[nd++] = batch;
                        check_coverage(ordered, n, qmask, sc, rounds, batch, hits);
                        ++cases;
                    }
                }
        }
    g_cases += cases;
}

int main() {
    std::atomic<int> next{kMaxTables};  // the long ones first
    std::vector<std::thread> pool;
    for (int i = 0; i < 8; ++i)
        pool.emplace_back([&] {
            for (int n; (n = next--) >= 2;) run_tables(n);
        });
    for (auto& t : pool) t.join();
    printf("%ld cases, %d failures\n", g_cases.load(), g_fail.load());
    return g_fail.load() ? 1 : 0;
}
