// Stand-alone check of csrc/et_lookup_order.h (built and run by tests/test_lookup_order_host.py
// with -fsanitize=address,undefined): the class-slot -> item maps and the host's entry orderings.
// For every ntables 2..32, nheavy 0..ntables, sc in {1, 2, 3, 65, 128} and every policy:
//   * per XCD, the claims h = 0 .. nk * sc - 1 of the two classes together hit every slot
//     j * ntables + k exactly once;
//   * h >= nk * sc yields kNone;
//   * every XCD's entry list is, class by class, a permutation of what place_stripes assigned
//     (placement unchanged), and the placement itself covers every (table, stripe) once.
#include <stdio.h>
#include <string.h>

#include <atomic>
#include <thread>
#include <vector>

#include "et_lookup_order.h"

using namespace et_order;

static std::atomic<int> g_fail{0};
static std::atomic<long> g_cases{0};
#define CHECK(cond, ...)                 \
    do {                                 \
        if (!(cond)) {                   \
            if (g_fail++ < 20) {         \
                printf("FAIL %s: ", #cond); \
                printf(__VA_ARGS__);     \
                printf("\n");            \
            }                            \
        }                                \
    } while (0)

static const int kSc[] = {1, 2, 3, 65, 128};
static const int64_t kLight = 4 << 20, kNt = 256ll << 20;

// Table sizes with `nheavy` tables above kLight, every second of them above kNt, in mixed order.
static void make_bytes(int n, int nheavy, int64_t* bytes, uint32_t* nt_mask) {
    *nt_mask = 0;
    int h = 0;
    for (int t = 0; t < n; ++t) {
        // heavy tables spread over the table ids: t * nheavy / n steps exactly nheavy times
        const bool heavy = (t + 1) * nheavy / n > t * nheavy / n;
        if (heavy) {
            const bool nt = (h++ & 1) == 0;
            bytes[t] = nt ? kNt + 512 * (t + 1) : kLight + 512 * (t + 1);
            if (nt) *nt_mask |= 1u << t;
        } else {
            // light: from 3 rows to just under 4 MiB, some above and some below 1 and 2 MiB
            bytes[t] = 512ll * (3 + (int64_t)((t * 2654435761u) % 8000u));
        }
    }
}

static bool same_multiset(const uint32_t* a, const uint32_t* b, int n) {
    std::vector<bool> used(n, false);
    for (int i = 0; i < n; ++i) {
        bool found = false;
        for (int k = 0; k < n && !found; ++k)
            if (!used[k] && b[k] == a[i]) used[k] = found = true;
        if (!found) return false;
    }
    return true;
}

static void check_maps(const ClassOrder ord[2], int n, int nh, const char* what) {
    for (int sc : kSc) {
        std::vector<int> hits((size_t)n * sc);
        for (int x = 0; x < kXcds; ++x) {
            std::fill(hits.begin(), hits.end(), 0);
            for (uint32_t c = 0; c < 2; ++c) {
                const uint32_t nk = c ? n - nh : nh;
                for (uint32_t h = 0; h < nk * sc; ++h) {
                    const uint32_t s = class_slot(ord[c], x, c, h, nh, n, sc);
                    CHECK(s != kNone && s < (uint32_t)(n * sc), "%s n %d nh %d sc %d x %d c %u h %u -> %u",
                          what, n, nh, sc, x, c, h, s);
                    if (s == kNone || s >= (uint32_t)(n * sc)) continue;
                    const uint32_t k = s % n;
                    CHECK(c ? k >= (uint32_t)nh : k < (uint32_t)nh, "%s class of slot: n %d nh %d c %u k %u",
                          what, n, nh, c, k);
                    ++hits[s];
                }
                for (uint32_t h = nk * sc; h < nk * sc + 3u * sc + 5u; ++h)
                    CHECK(class_slot(ord[c], x, c, h, nh, n, sc) == kNone, "%s past the end: n %d nh %d sc %d h %u",
                          what, n, nh, sc, h);
                CHECK(class_slot(ord[c], x, c, ~0u - 1u, nh, n, sc) == kNone, "%s huge h", what);
            }
            for (size_t s = 0; s < hits.size(); ++s)
                CHECK(hits[s] == 1, "%s n %d nh %d sc %d x %d slot %zu hit %d times", what, n, nh, sc,
                      x, s, hits[s]);
        }
    }
}

// Every case with n tables.
static void run_tables(int n) {
    long cases = 0;
    {
        for (int nheavy = 0; nheavy <= n; ++nheavy) {
            int64_t bytes[kMaxTables];
            uint32_t nt_mask;
            make_bytes(n, nheavy, bytes, &nt_mask);
            uint32_t base[kXcds][kMaxEntries];
            int nh = -1;
            const int nent = place_stripes(bytes, n, kLight, base, &nh);
            CHECK(nent == n && nh == nheavy, "placement: n %d nheavy %d -> nent %d nh %d", n, nheavy,
                  nent, nh);
            // the placement itself: every (table, stripe) once on the chip; a heavy table's stripe
            // x on XCD x; each XCD lists its heavy entries first
            int seen[kMaxTables][kXcds];
            memset(seen, 0, sizeof(seen));
            for (int x = 0; x < kXcds; ++x)
                for (int k = 0; k < nent; ++k) {
                    const uint32_t t = entry_table(base[x][k]), st = (base[x][k] >> 8) & 0xffu;
                    CHECK(t < (uint32_t)n && st < (uint32_t)kXcds, "entry %08x", base[x][k]);
                    if (t >= (uint32_t)n || st >= (uint32_t)kXcds) continue;
                    ++seen[t][st];
                    const bool heavy = bytes[t] > kLight;
                    CHECK(heavy == (k < nh), "class boundary: x %d k %d", x, k);
                    if (heavy) CHECK(st == (uint32_t)x, "heavy stripe: x %d st %u", x, st);
                }
            for (int t = 0; t < n; ++t)
                for (int st = 0; st < kXcds; ++st)
                    CHECK(seen[t][st] == 1, "n %d nheavy %d (table %d, stripe %d) placed %d times", n,
                          nheavy, t, st, seen[t][st]);

            // both maps over the unordered entries, every split
            for (int major = 0; major < 4; ++major)
                for (int split : {major * n / 3}) {  // + x below: every XCD another split
                    ClassOrder ord[2];
                    for (int x = 0; x < kXcds; ++x) {
                        ord[0].split[x] = ord[1].split[x] = (uint8_t)((split + x) % (n + 2));
                        ord[0].major[x] = (uint8_t)major;
                        ord[1].major[x] = (uint8_t)(3 - major);
                    }
                    check_maps(ord, n, nh, "maps");
                    ++cases;
                }

            // every policy's host ordering
            for (int cache_major = 0; cache_major < 2; ++cache_major)
                for (int fab = 0; fab < 4; ++fab)
                    for (int64_t phase : {(int64_t)0, (int64_t)1 << 20, (int64_t)2 << 20, (int64_t)1 << 40}) {
                        if (fab != 1 && fab != 2 && phase != 0) continue;  // only (b) reads it
                        Policy p;
                        p.cache_major = cache_major;
                        p.fab = fab;
                        p.phase_bytes = phase;
                        uint32_t e[kXcds][kMaxEntries];
                        memcpy(e, base, sizeof(e));
                        ClassOrder ord[2];
                        memset(ord, 0xff, sizeof(ord));
                        for (int x = 0; x < kXcds; ++x) {
                            order_xcd(e[x], x, nent, nh, bytes, nt_mask, p, ord);
                            CHECK(same_multiset(e[x], base[x], nh), "fabric entries moved: n %d nh %d x %d", n,
                                  nh, x);
                            CHECK(same_multiset(e[x] + nh, base[x] + nh, nent - nh),
                                  "cache entries moved: n %d nh %d x %d", n, nh, x);
                            CHECK(ord[0].split[x] <= nh && ord[1].split[x] <= nent - nh, "split");
                            if (cache_major)  // largest first
                                for (int k = nh + 1; k < nent; ++k)
                                    CHECK(bytes[entry_table(e[x][k - 1])] >= bytes[entry_table(e[x][k])],
                                          "cache order x %d k %d", x, k);
                            if (fab == 1 || fab == 2) {  // two phases, split at the boundary
                                const bool nt0 = nh > 0 && ((nt_mask >> entry_table(e[x][0])) & 1u);
                                for (int k = 0; k < nh; ++k) {
                                    const bool nt = (nt_mask >> entry_table(e[x][k])) & 1u;
                                    const bool first = k < ord[0].split[x];
                                    if (ord[0].split[x] > 0 && ord[0].split[x] < nh)
                                        CHECK(nt == (first ? nt0 : !nt0), "phases x %d k %d", x, k);
                                }
                            }
                        }
                        if (!cache_major && !fab) {  // the default policy changes nothing
                            CHECK(memcmp(e, base, sizeof(e)) == 0, "default policy moved entries");
                            ClassOrder zero[2];
                            memset(zero, 0, sizeof(zero));
                            CHECK(memcmp(ord, zero, sizeof(zero)) == 0, "default policy order");
                        }
                        check_maps(ord, nent, nh, "policy");
                        ++cases;
                    }
        }
    }
    g_cases += cases;
}

int main() {
    // the table counts are independent: a few host threads share them (the divisions of the map
    // make one thread take ten seconds under the sanitizers)
    std::atomic<int> next{kMaxTables};  // the long ones first
    std::vector<std::thread> pool;
    for (int i = 0; i < 8; ++i)
        pool.emplace_back([&] {
            for (int n; (n = next--) >= 2;) run_tables(n);
        });
    for (auto& t : pool) t.join();
    // the default order is the static one: tables fastest within the class
    ClassOrder zero[2];
    memset(zero, 0, sizeof(zero));
    for (uint32_t h = 0; h < 7 * 7; ++h) {
        if (h < 5 * 7)
            CHECK(class_slot(zero[0], 3, 0, h, 5, 12, 7) == (h / 5) * 12 + h % 5, "static fabric h %u", h);
        CHECK(class_slot(zero[1], 3, 1, h, 5, 12, 7) == (h / 7) * 12 + 5 + h % 7, "static cache h %u", h);
    }
    printf("%ld cases, %d failures\n", g_cases.load(), g_fail.load());
    return g_fail.load() ? 1 : 0;
}
