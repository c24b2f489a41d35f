// et_weighted.hip — weighted and mean-pooled bags (et_weighted_maplookup_prealloc) and the
// gradient with respect to the weights (et_weighted_weight_grad), textually included by
// et_lookup.hip inside namespace et: it reuses VecGeom, idx_row32, pack16 / unpack16, col_ptr,
// ragged_range, the store helpers and note_oob of that translation unit.
//
// The reference has no weighted form; include/embtab.h states the arithmetic.  C is the
// accumulator type (float for F32 / F16 / BF16 tables, double for F64); weights and weight
// gradients are of type C.  Forward, for a bag [lo, hi): acc = C(w_lo) * C(x_lo), then
// t = C(w_k) * C(x_k), acc = acc + t for the other entries in index order (two roundings, the
// library is built with -ffp-contract=off), out = T(acc).  Without weights the sum starts
// from a copy of the first row (k_ragged_vec's result with fp32 accumulation, bit for bit);
// mean mode divides that sum by C(hi - lo) once.
//
// Geometry: k_ragged_vec's.  The lane that loads index slot c0 + sub also
// loads that slot's weight; both reach the lane group through a per-lane shuffle
// (ds_bpermute), because the loop counters of a wave's groups differ.  Lanes past the bag's
// end re-read the last slot, so no weight outside a bag's clamped range is ever read.

struct WeightedPack {
    et_weighted_desc d[ET_MAX_TABLES_PER_LAUNCH];
};

// One rounding from the accumulator to a 16-bit element.  The empty asm keeps the compiler
// from folding fptrunc(w * x) (a one-entry bag) or fptrunc(acc + t) into a mixed-precision
// instruction that rounds the exact result to 16 bits once (sgd_apply_t's barrier).
template <typename T, typename C>
__device__ __forceinline__ T weighted_round(C a) {
    if constexpr (sizeof(T) == 2 && __is_same(C, float)) {
        asm volatile("" : "+v"(a));
    }
    return T(a);
}

// UU rows of one bag (ragged_load_add with a weight per slot): every load is issued before
// the first product, then the rows are multiplied and added in slot order.  `myw` is the
// weight of the slot whose index this lane loaded (W only).
template <typename T, typename C, int D, int UU, bool W>
__device__ __forceinline__ void weighted_load_add(const T* __restrict__ table, uint32_t ld_table,
                                                  uint32_t cpp, uint32_t myr, C myw, int gbase,
                                                  int sub, int i0, bool first,
                                                  C (&acc)[VecGeom<T, D>::NV][VecGeom<T, D>::N],
                                                  int& bad, int vpr) {
    using G = VecGeom<T, D>;
    constexpr int N = G::N, LPR = G::LPR, NV = G::NV;
    const u32x4* src[UU];
    bool ok[UU];
    C w[UU];
#pragma unroll
    for (int u = 0; u < UU; ++u) {
        const uint32_t r = (uint32_t)__shfl((int)myr, gbase + i0 + u, 64);
        if constexpr (W) w[u] = __shfl(myw, gbase + i0 + u, 64);
        ok[u] = r != ~0u;
        const uint32_t row32 = ok[u] ? r : 0u;
        if (cpp != 0u) {
            const uint32_t page = row32 / cpp;
            src[u] = reinterpret_cast<const u32x4*>(
                reinterpret_cast<const T* const*>(table)[page] +
                (uint64_t)(row32 - page * cpp) * ld_table);
        } else {
            src[u] = reinterpret_cast<const u32x4*>(table + (uint64_t)row32 * ld_table);
        }
    }
    int vix[NV];  // lanes beyond the row re-read its last vector (in bounds) and never store
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        vix[v] = sub + v * LPR;
        vix[v] = vix[v] < vpr ? vix[v] : vpr - 1;
    }
    u32x4 buf[UU][NV];
#pragma unroll
    for (int u = 0; u < UU; ++u)
#pragma unroll
        for (int v = 0; v < NV; ++v) buf[u][v] = src[u][vix[v]];
#pragma unroll
    for (int u = 0; u < UU; ++u) {
        bad += ok[u] ? 0 : 1;
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            T x[N];
            unpack16<T, N>(ok[u] ? buf[u][v] : u32x4{0u, 0u, 0u, 0u}, x);
#pragma unroll
            for (int k = 0; k < N; ++k) {
                C t = C(x[k]);
                if constexpr (W) t = w[u] * t;  // an out-of-range row is +0, still multiplied
                if (u == 0)
                    acc[v][k] = first ? t : C(acc[v][k] + t);
                else
                    acc[v][k] = C(acc[v][k] + t);
            }
        }
    }
}

// Weighted / mean pooled sum, vector path: any row that is a multiple of 16 bytes, at the
// power-of-two capacity D of its dim.  W: the group's tables carry weights (sum mode);
// otherwise each table's own mode says sum or mean.  Grid as k_ragged_vec.
template <typename T, typename C, int D, bool W>
__global__ __launch_bounds__(256) void k_weighted_vec(WeightedPack pack, int ntables,
                                                      int64_t batch, T* __restrict__ dst,
                                                      int64_t ld_dst, int nt) {
    using G = VecGeom<T, D>;
    constexpr int N = G::N, LPR = G::LPR, NV = G::NV, U = G::U;
    const int64_t item = blockIdx.x;
    const int t = (int)(item % ntables);
    const int64_t chunk = item / ntables;
    const et_weighted_desc& d = pack.d[t];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = lane / LPR, sub = lane % LPR, gbase = g * LPR;
    const int64_t bag = chunk * (4 * G::GPW) + wave * G::GPW + g;
    if (bag >= batch) return;
    const T* table = reinterpret_cast<const T*>(d.table);
    const uint32_t ldt = (uint32_t)d.ld_table, nr = (uint32_t)d.nrows;
    const uint32_t cpp = (uint32_t)d.cols_per_page;
    const int vpr = d.dim / N;
    int64_t lo, hi;
    int bad;
    ragged_range(d.colptr, bag, d.nnz, lo, hi, bad);
    const int64_t* __restrict__ ip = d.idx + lo;
    const C* __restrict__ wp = reinterpret_cast<const C*>(d.weights) + lo;
    const int64_t len = hi - lo;

    C acc[NV][N];
#pragma unroll
    for (int v = 0; v < NV; ++v)
#pragma unroll
        for (int k = 0; k < N; ++k) acc[v][k] = C(0);

    for (int64_t c0 = 0; c0 < len; c0 += LPR) {
        const int cnt = len - c0 < LPR ? (int)(len - c0) : LPR;
        // one index and its weight per lane; lanes past the end re-read the last slot
        const int64_t slot = c0 + (sub < cnt ? sub : cnt - 1);
        const uint32_t myr = idx_row32((long long)ip[slot], nr);
        C myw = C(0);
        if constexpr (W) myw = wp[slot];
        int i0 = 0;
#define ET_WT_LOAD_ADD(UU)                                                                  \
    weighted_load_add<T, C, D, UU, W>(table, ldt, cpp, myr, myw, gbase, sub, i0,            \
                                      c0 == 0 && i0 == 0, acc, bad, vpr)
        for (; i0 + U <= cnt; i0 += U) ET_WT_LOAD_ADD(U);
        if constexpr (U > 4) {
            if (cnt - i0 >= 4) {
                ET_WT_LOAD_ADD(4);
                i0 += 4;
            }
        }
        if constexpr (U > 2) {
            if (cnt - i0 >= 2) {
                ET_WT_LOAD_ADD(2);
                i0 += 2;
            }
        }
        if constexpr (U > 1) {
            if (cnt - i0 >= 1) ET_WT_LOAD_ADD(1);
        }
#undef ET_WT_LOAD_ADD
    }
    if (bad && sub == 0) note_oob(bad);
    const bool mean = !W && d.mode == ET_POOL_MEAN && len > 0;
    const C flen = C(len);
    u32x4* o = reinterpret_cast<u32x4*>(dst + bag * ld_dst + d.dst_row_off) + sub;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        T y[N];
#pragma unroll
        for (int k = 0; k < N; ++k)
            y[k] = weighted_round<T, C>(mean ? C(acc[v][k] / flen) : acc[v][k]);
        if (sub + v * LPR < vpr) {
            if (nt)
                store16<true>(o + v * LPR, pack16<T, N>(y));
            else
                store16<false>(o + v * LPR, pack16<T, N>(y));
        }
    }
}

// Generic path (k_ragged_generic with weights): any dim / alignment, paged and
// column-pointer tables through col_ptr.  One wave per bag, lanes stride over the features,
// the bag's entries sequential per feature.  The weight of an entry is a wave-uniform load.
template <typename T, typename C, bool W>
__global__ __launch_bounds__(256) void k_weighted_generic(WeightedPack pack, int ntables,
                                                          int64_t batch, T* __restrict__ dst,
                                                          int64_t ld_dst, int nt) {
    constexpr int K = 4;
    const int64_t item = blockIdx.x;
    const int t = (int)(item % ntables);
    const int64_t chunk = item / ntables;
    const et_weighted_desc& d = pack.d[t];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t bag = chunk * 4 + wave;
    if (bag >= batch) return;
    int64_t lo, hi;
    int clamped;
    ragged_range(d.colptr, bag, d.nnz, lo, hi, clamped);
    if (clamped && lane == 0) note_oob(clamped);
    T* out = dst + bag * ld_dst + d.dst_row_off;
    const C* __restrict__ wp = reinterpret_cast<const C*>(d.weights);
    const int dim = d.dim;
    const bool mean = !W && d.mode == ET_POOL_MEAN && hi > lo;
    const C flen = C(hi - lo);
    for (int f0 = 0; f0 < dim; f0 += 64 * K) {
        C acc[K];
#pragma unroll
        for (int k = 0; k < K; ++k) acc[k] = C(0);
        for (int64_t i = lo; i < hi; ++i) {
            uint64_t row = (uint64_t)(d.idx[i] - 1);
            const bool ok = row < (uint64_t)d.nrows;
            if (!ok && lane == 0 && f0 == 0) note_oob();
            row = ok ? row : 0;
            const T* src = col_ptr<const T>(d.table, d.ld_table, d.cols_per_page, row);
            C w = C(1);
            if constexpr (W) w = wp[i];
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const int f = f0 + lane + 64 * k;
                if (f < dim) {
                    C x = ok ? C(src[f]) : C(0);
                    if constexpr (W) x = w * x;
                    acc[k] = i == lo ? x : C(acc[k] + x);
                }
            }
        }
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int f = f0 + lane + 64 * k;
            if (f < dim) {
                const T y = weighted_round<T, C>(mean ? C(acc[k] / flen) : acc[k]);
                if (nt)
                    store_scalar<true>(out + f, y);
                else
                    store_scalar<false>(out + f, y);
            }
        }
    }
}

// ---------------------------------------------------------------------------
// Weight gradient: dw[k] = sum_f C(delta[f, bag(k)]) * C(x_k[f])
// ---------------------------------------------------------------------------

struct WeightGradPack {
    et_weighted_update_desc d[ET_MAX_TABLES_PER_LAUNCH];
};

// UU entries of one bag: load their rows, multiply by the bag's gradient column `gc` (held in
// registers), sum the lane's products in (vector, element) order, then reduce across the
// group with __shfl_xor butterflies — a fixed order, the same from run to run.  The lane
// whose sub equals the entry's slot keeps the result in `mine`.
template <typename T, typename C, int D, int UU>
__device__ __forceinline__ void wgrad_rows(const T* __restrict__ table, uint32_t ld_table,
                                           uint32_t cpp, uint32_t myr, int gbase, int sub, int i0,
                                           const C (&gc)[VecGeom<T, D>::NV][VecGeom<T, D>::N],
                                           C& mine, int& bad, int vpr) {
    using G = VecGeom<T, D>;
    constexpr int N = G::N, LPR = G::LPR, NV = G::NV;
    const u32x4* src[UU];
    bool ok[UU];
#pragma unroll
    for (int u = 0; u < UU; ++u) {
        const uint32_t r = (uint32_t)__shfl((int)myr, gbase + i0 + u, 64);
        ok[u] = r != ~0u;
        const uint32_t row32 = ok[u] ? r : 0u;
        if (cpp != 0u) {
            const uint32_t page = row32 / cpp;
            src[u] = reinterpret_cast<const u32x4*>(
                reinterpret_cast<const T* const*>(table)[page] +
                (uint64_t)(row32 - page * cpp) * ld_table);
        } else {
            src[u] = reinterpret_cast<const u32x4*>(table + (uint64_t)row32 * ld_table);
        }
    }
    int vix[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        vix[v] = sub + v * LPR;
        vix[v] = vix[v] < vpr ? vix[v] : vpr - 1;
    }
    u32x4 buf[UU][NV];
#pragma unroll
    for (int u = 0; u < UU; ++u)
#pragma unroll
        for (int v = 0; v < NV; ++v) buf[u][v] = src[u][vix[v]];
#pragma unroll
    for (int u = 0; u < UU; ++u) {
        bad += ok[u] ? 0 : 1;
        C p = C(0);
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            T x[N];
            // lanes beyond the row hold a re-read vector: it contributes +0 * +0
            const bool in = sub + v * LPR < vpr;
            unpack16<T, N>(in ? buf[u][v] : u32x4{0u, 0u, 0u, 0u}, x);
#pragma unroll
            for (int k = 0; k < N; ++k) p = p + gc[v][k] * C(x[k]);
        }
#pragma unroll
        for (int m = LPR / 2; m >= 1; m >>= 1) p = p + __shfl_xor(p, m, 64);
        if (sub == i0 + u) mine = ok[u] ? p : C(0);  // an out-of-range index gives +0
    }
}

// Weight gradient, vector path: bag-major in k_weighted_vec's geometry.  A lane group loads
// its bag's gradient column once (NV * N values converted to C), walks the bag's entries
// with U rows in flight and stores one dw per entry (lane `slot` of the group stores slot
// `slot` of the chunk, a contiguous store).  No LDS, no barrier, no bag-id array.
template <typename T, typename C, int D>
__global__ __launch_bounds__(256) void k_weight_grad_vec(WeightGradPack pack, int ntables) {
    using G = VecGeom<T, D>;
    constexpr int N = G::N, LPR = G::LPR, NV = G::NV, U = G::U;
    const int64_t item = blockIdx.x;
    const int t = (int)(item % ntables);
    const int64_t chunk = item / ntables;
    const et_weighted_update_desc& d = pack.d[t];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = lane / LPR, sub = lane % LPR, gbase = g * LPR;
    const int64_t bag = chunk * (4 * G::GPW) + wave * G::GPW + g;
    if (bag >= d.batch) return;
    const T* table = reinterpret_cast<const T*>(d.table);
    const uint32_t ldt = (uint32_t)d.ld_table, nr = (uint32_t)d.nrows;
    const uint32_t cpp = (uint32_t)d.cols_per_page;
    const int vpr = d.dim / N;
    int64_t lo, hi;
    int bad;
    ragged_range(d.colptr, bag, d.nnz, lo, hi, bad);
    const int64_t len = hi - lo;
    if (len == 0) {
        if (bad && sub == 0) note_oob(bad);
        return;
    }
    const int64_t* __restrict__ ip = d.idx + lo;
    C* __restrict__ dw = reinterpret_cast<C*>(d.dweights) + lo;

    C gc[NV][N];
    const u32x4* gp = reinterpret_cast<const u32x4*>(reinterpret_cast<const T*>(d.delta) +
                                                     bag * d.ld_delta);
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        const int ix = sub + v * LPR;
        T x[N];
        unpack16<T, N>(ix < vpr ? gp[ix] : u32x4{0u, 0u, 0u, 0u}, x);
#pragma unroll
        for (int k = 0; k < N; ++k) gc[v][k] = C(x[k]);
    }

    for (int64_t c0 = 0; c0 < len; c0 += LPR) {
        const int cnt = len - c0 < LPR ? (int)(len - c0) : LPR;
        const uint32_t myr = idx_row32((long long)ip[c0 + (sub < cnt ? sub : cnt - 1)], nr);
        C mine = C(0);
        int i0 = 0;
#define ET_WG_ROWS(UU) \
    wgrad_rows<T, C, D, UU>(table, ldt, cpp, myr, gbase, sub, i0, gc, mine, bad, vpr)
        for (; i0 + U <= cnt; i0 += U) ET_WG_ROWS(U);
        if constexpr (U > 4) {
            if (cnt - i0 >= 4) {
                ET_WG_ROWS(4);
                i0 += 4;
            }
        }
        if constexpr (U > 2) {
            if (cnt - i0 >= 2) {
                ET_WG_ROWS(2);
                i0 += 2;
            }
        }
        if constexpr (U > 1) {
            if (cnt - i0 >= 1) ET_WG_ROWS(1);
        }
#undef ET_WG_ROWS
        if (sub < cnt) dw[c0 + sub] = mine;
    }
    if (bad && sub == 0) note_oob(bad);
}

// Generic weight gradient: one wave per bag, the entries one after another, lanes stride over
// the features (each lane sums its products in feature order), then a butterfly over the wave.
template <typename T, typename C>
__global__ __launch_bounds__(256) void k_weight_grad_generic(WeightGradPack pack, int ntables) {
    const int64_t item = blockIdx.x;
    const int t = (int)(item % ntables);
    const int64_t chunk = item / ntables;
    const et_weighted_update_desc& d = pack.d[t];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t bag = chunk * 4 + wave;
    if (bag >= d.batch) return;
    int64_t lo, hi;
    int clamped;
    ragged_range(d.colptr, bag, d.nnz, lo, hi, clamped);
    if (clamped && lane == 0) note_oob(clamped);
    const T* __restrict__ gcol = reinterpret_cast<const T*>(d.delta) + bag * d.ld_delta;
    C* __restrict__ dw = reinterpret_cast<C*>(d.dweights);
    const int dim = d.dim;
    for (int64_t i = lo; i < hi; ++i) {
        uint64_t row = (uint64_t)(d.idx[i] - 1);
        const bool ok = row < (uint64_t)d.nrows;
        if (!ok && lane == 0) note_oob();
        row = ok ? row : 0;
        const T* src = col_ptr<const T>(d.table, d.ld_table, d.cols_per_page, row);
        C p = C(0);
        for (int f = lane; f < dim; f += 64) p = p + C(gcol[f]) * C(src[f]);
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) p = p + __shfl_xor(p, m, 64);
        if (lane == 0) dw[i] = ok ? p : C(0);
    }
}

// ---------------------------------------------------------------------------
// Host dispatch
// ---------------------------------------------------------------------------

template <typename T, typename C, int D>
int launch_weighted_vec_d(bool w, const WeightedPack& pack, int n, int64_t batch, void* dst,
                          int64_t ld_dst, bool nt, hipStream_t s) {
    const int64_t per = 4 * VecGeom<T, D>::GPW;
    const int64_t grid = (batch + per - 1) / per * n;
    if (grid > 0x7fffffffll) return fail(ET_ERR_ARG, "grid too large");
    if (w)
        hipLaunchKernelGGL((k_weighted_vec<T, C, D, true>), dim3((unsigned)grid), dim3(256), 0, s,
                           pack, n, batch, reinterpret_cast<T*>(dst), ld_dst, nt ? 1 : 0);
    else
        hipLaunchKernelGGL((k_weighted_vec<T, C, D, false>), dim3((unsigned)grid), dim3(256), 0,
                           s, pack, n, batch, reinterpret_cast<T*>(dst), ld_dst, nt ? 1 : 0);
    ET_LAUNCH_CHECK("k_weighted_vec");
    return ET_OK;
}

template <typename T, typename C>
int launch_weighted_typed(bool vec, bool w, const WeightedPack& pack, int n, int D, int64_t batch,
                          void* dst, int64_t ld_dst, bool nt, hipStream_t s) {
    if (vec) {
#define ET_WT(CAP)                                                                          \
    case CAP:                                                                               \
        if constexpr (CAP / (16 / (int)sizeof(T)) >= 1)                                     \
            return launch_weighted_vec_d<T, C, CAP>(w, pack, n, batch, dst, ld_dst, nt, s); \
        break;
        switch (masked_capacity(D)) {
            ET_WT(16)
            ET_WT(32)
            ET_WT(64)
            ET_WT(128)
            ET_WT(256)
            ET_WT(512)
            ET_WT(1024)
            ET_WT(2048)
        }
#undef ET_WT
        return fail(ET_ERR_UNSUPPORTED, "weighted vector dim %d", D);
    }
    const int64_t grid = (batch + 3) / 4 * n;
    if (grid > 0x7fffffffll) return fail(ET_ERR_ARG, "grid too large");
    if (w)
        hipLaunchKernelGGL((k_weighted_generic<T, C, true>), dim3((unsigned)grid), dim3(256), 0, s,
                           pack, n, batch, reinterpret_cast<T*>(dst), ld_dst, nt ? 1 : 0);
    else
        hipLaunchKernelGGL((k_weighted_generic<T, C, false>), dim3((unsigned)grid), dim3(256), 0,
                           s, pack, n, batch, reinterpret_cast<T*>(dst), ld_dst, nt ? 1 : 0);
    ET_LAUNCH_CHECK("k_weighted_generic");
    return ET_OK;
}

inline bool weighted_dtype_ok(int dtype) {
    return dtype == ET_F32 || dtype == ET_F64 || dtype == ET_F16 || dtype == ET_BF16;
}

// Validate everything, then group the tables by (kernel, capacity, weights or none) and
// launch one kernel per group.
inline int weighted_dispatch(int dtype, const et_weighted_desc* descs, int ntables, int64_t batch,
                             void* dst, int64_t ld_dst, uint32_t flags, hipStream_t s) {
    const int es = elsize(dtype);
    if (es == 0) return fail(ET_ERR_UNSUPPORTED, "unknown dtype %d", dtype);
    if (!weighted_dtype_ok(dtype))
        return fail(ET_ERR_UNSUPPORTED, "weighted lookup: dtype %d (float tables only)", dtype);
    if (flags & ~ET_FLAG_NONTEMPORAL)
        return fail(ET_ERR_UNSUPPORTED, "weighted lookup: flags 0x%x (non-temporal stores only)",
                    flags);
    if (ntables < 0 || batch < 0) return fail(ET_ERR_ARG, "negative ntables/batch");
    if (ntables > ET_MAX_TABLES_PER_LAUNCH)
        return fail(ET_ERR_ARG, "at most %d tables per weighted lookup", ET_MAX_TABLES_PER_LAUNCH);
    if (ntables == 0 || batch == 0) return ET_OK;
    if (batch >= 0x7fffffffll) return fail(ET_ERR_ARG, "batch too large");
    if (!descs) return fail(ET_ERR_ARG, "descs is NULL");
    if (!dst) return fail(ET_ERR_ARG, "dst is NULL");
    const int ws = dtype == ET_F64 ? 8 : 4;
    int kind_of[ET_MAX_TABLES_PER_LAUNCH];  // -1 nothing; bit 0 vector, bit 1 weights
    for (int t = 0; t < ntables; ++t) {
        const et_weighted_desc& d = descs[t];
        if (d.dim < 0 || d.nrows < 0 || d.nnz < 0 || d.cols_per_page < 0)
            return fail(ET_ERR_ARG, "table %d: negative dim/nrows/nnz/cols_per_page", t);
        if (d.mode != ET_POOL_SUM && d.mode != ET_POOL_MEAN)
            return fail(ET_ERR_ARG, "table %d: mode %d", t, d.mode);
        if (d.mode == ET_POOL_MEAN && d.weights)
            return fail(ET_ERR_UNSUPPORTED, "table %d: weights with mean pooling", t);
        if (d.dim == 0) {
            kind_of[t] = -1;
            continue;
        }
        if (d.ld_table < d.dim) return fail(ET_ERR_ARG, "table %d: ld_table < dim", t);
        if (d.dst_row_off < 0 || d.dst_row_off + d.dim > ld_dst)
            return fail(ET_ERR_ARG, "table %d: rows [%lld, %lld) outside ld_dst %lld", t,
                        (long long)d.dst_row_off, (long long)(d.dst_row_off + d.dim),
                        (long long)ld_dst);
        if (!d.colptr) return fail(ET_ERR_ARG, "table %d: NULL colptr", t);
        if (d.nnz > 0) {
            if (!d.table || !d.idx) return fail(ET_ERR_ARG, "table %d: NULL table/idx", t);
            if (d.nrows == 0) return fail(ET_ERR_ARG, "table %d: indices into an empty table", t);
        }
        if (d.weights && (reinterpret_cast<uintptr_t>(d.weights) % ws) != 0)
            return fail(ET_ERR_ARG, "table %d: weights not aligned to their element type", t);
        const bool al = ((d.ld_table * es) % 16 == 0) && ((int64_t)d.dim * es) % 16 == 0 &&
                        (d.cols_per_page > 0 || aligned16(d.table)) &&
                        aligned16(static_cast<char*>(dst) + d.dst_row_off * es) &&
                        ((ld_dst * es) % 16 == 0);
        const bool vec = al && d.dim <= 2048 && d.nnz > 0 && d.nrows < 0xffffffffll &&
                         d.ld_table < 0xffffffffll && d.cols_per_page < 0xffffffffll;
        kind_of[t] = (vec ? 1 : 0) | (d.weights ? 2 : 0);
    }
    const bool nt = (flags & ET_FLAG_NONTEMPORAL) != 0;
    bool done[ET_MAX_TABLES_PER_LAUNCH] = {false};
    for (int t0 = 0; t0 < ntables; ++t0) {
        if (done[t0] || kind_of[t0] < 0) continue;
        WeightedPack pack;
        int n = 0;
        const bool vec = (kind_of[t0] & 1) != 0, w = (kind_of[t0] & 2) != 0;
        const int cap = vec ? masked_capacity(descs[t0].dim) : 0;
        for (int t = t0; t < ntables; ++t) {
            if (done[t] || kind_of[t] != kind_of[t0]) continue;
            if (vec && masked_capacity(descs[t].dim) != cap) continue;
            pack.d[n++] = descs[t];
            done[t] = true;
        }
        int rc;
        switch (dtype) {
            case ET_F32:
                rc = launch_weighted_typed<float, float>(vec, w, pack, n, cap, batch, dst, ld_dst,
                                                         nt, s);
                break;
            case ET_F64:
                rc = launch_weighted_typed<double, double>(vec, w, pack, n, cap, batch, dst,
                                                           ld_dst, nt, s);
                break;
            case ET_BF16:
                rc = launch_weighted_typed<__bf16, float>(vec, w, pack, n, cap, batch, dst, ld_dst,
                                                          nt, s);
                break;
            default:  // ET_F16
                rc = launch_weighted_typed<_Float16, float>(vec, w, pack, n, cap, batch, dst,
                                                            ld_dst, nt, s);
        }
        if (rc != ET_OK) return rc;
    }
    return ET_OK;
}

template <typename T, typename C>
int launch_weight_grad_typed(bool vec, const WeightGradPack& pack, int n, int D, int64_t batch,
                             hipStream_t s) {
    if (vec) {
#define ET_WG(CAP)                                                                              \
    case CAP:                                                                                   \
        if constexpr (CAP / (16 / (int)sizeof(T)) >= 1) {                                       \
            const int64_t per = 4 * VecGeom<T, CAP>::GPW;                                       \
            const int64_t grid = (batch + per - 1) / per * n;                                   \
            if (grid > 0x7fffffffll) return fail(ET_ERR_ARG, "grid too large");                 \
            hipLaunchKernelGGL((k_weight_grad_vec<T, C, CAP>), dim3((unsigned)grid), dim3(256), \
                               0, s, pack, n);                                                  \
            ET_LAUNCH_CHECK("k_weight_grad_vec");                                               \
            return ET_OK;                                                                       \
        }                                                                                       \
        break;
        switch (masked_capacity(D)) {
            ET_WG(16)
            ET_WG(32)
            ET_WG(64)
            ET_WG(128)
            ET_WG(256)
            ET_WG(512)
            ET_WG(1024)
            ET_WG(2048)
        }
#undef ET_WG
        return fail(ET_ERR_UNSUPPORTED, "weight gradient vector dim %d", D);
    }
    const int64_t grid = (batch + 3) / 4 * n;
    if (grid > 0x7fffffffll) return fail(ET_ERR_ARG, "grid too large");
    hipLaunchKernelGGL((k_weight_grad_generic<T, C>), dim3((unsigned)grid), dim3(256), 0, s, pack,
                       n);
    ET_LAUNCH_CHECK("k_weight_grad_generic");
    return ET_OK;
}

inline int weight_grad_dispatch(int dtype, const et_weighted_update_desc* descs, int ntables,
                                hipStream_t s) {
    if (!weighted_dtype_ok(dtype))
        return fail(ET_ERR_UNSUPPORTED, "weight gradient: dtype %d (float tables only)", dtype);
    if (ntables < 0) return fail(ET_ERR_ARG, "negative ntables");
    if (ntables > ET_MAX_TABLES_PER_LAUNCH)
        return fail(ET_ERR_ARG, "at most %d tables per call", ET_MAX_TABLES_PER_LAUNCH);
    if (ntables == 0) return ET_OK;
    if (!descs) return fail(ET_ERR_ARG, "descs is NULL");
    const int es = elsize(dtype), ws = dtype == ET_F64 ? 8 : 4;
    int kind_of[ET_MAX_TABLES_PER_LAUNCH];  // -1 nothing to launch, 0 generic, 1 vector
    for (int t = 0; t < ntables; ++t) {
        const et_weighted_update_desc& d = descs[t];
        if (d.dim < 0 || d.nrows < 0 || d.nnz < 0 || d.batch < 0 || d.cols_per_page < 0)
            return fail(ET_ERR_ARG, "table %d: negative size", t);
        if (d.batch >= 0x7fffffffll) return fail(ET_ERR_ARG, "table %d: batch too large", t);
        kind_of[t] = -1;
        if (d.nnz == 0) continue;
        if (!d.dweights) return fail(ET_ERR_ARG, "table %d: NULL dweights", t);
        if ((reinterpret_cast<uintptr_t>(d.dweights) % ws) != 0)
            return fail(ET_ERR_ARG, "table %d: dweights not aligned to their element type", t);
        if (d.batch == 0 || d.dim == 0) continue;  // every entry +0: the memset alone
        if (!d.idx || !d.colptr || !d.table || !d.delta)
            return fail(ET_ERR_ARG, "table %d: NULL", t);
        if (d.nrows == 0) return fail(ET_ERR_ARG, "table %d: indices into an empty table", t);
        if (d.ld_table < d.dim || d.ld_delta < d.dim)
            return fail(ET_ERR_ARG, "table %d: leading dimension < dim", t);
        const bool al = ((d.ld_table * es) % 16 == 0) && ((int64_t)d.dim * es) % 16 == 0 &&
                        (d.cols_per_page > 0 || aligned16(d.table)) && aligned16(d.delta) &&
                        ((d.ld_delta * es) % 16 == 0);
        const bool vec = al && d.dim <= 2048 && d.nrows < 0xffffffffll &&
                         d.ld_table < 0xffffffffll && d.cols_per_page < 0xffffffffll;
        kind_of[t] = vec ? 1 : 0;
    }
    // entries no bag covers (and tables with nothing to launch) are +0
    for (int t = 0; t < ntables; ++t)
        if (descs[t].nnz > 0)
            ET_HIP_CHECK(hipMemsetAsync(descs[t].dweights, 0, (size_t)descs[t].nnz * ws, s));
    bool done[ET_MAX_TABLES_PER_LAUNCH] = {false};
    for (int t0 = 0; t0 < ntables; ++t0) {
        if (done[t0] || kind_of[t0] < 0) continue;
        WeightGradPack pack;
        int n = 0;
        int64_t batch = 0;
        const bool vec = kind_of[t0] == 1;
        const int cap = vec ? masked_capacity(descs[t0].dim) : 0;
        for (int t = t0; t < ntables; ++t) {
            if (done[t] || kind_of[t] != kind_of[t0]) continue;
            if (vec && masked_capacity(descs[t].dim) != cap) continue;
            pack.d[n++] = descs[t];
            if (descs[t].batch > batch) batch = descs[t].batch;
            done[t] = true;
        }
        int rc;
        switch (dtype) {
            case ET_F32:
                rc = launch_weight_grad_typed<float, float>(vec, pack, n, cap, batch, s);
                break;
            case ET_F64:
                rc = launch_weight_grad_typed<double, double>(vec, pack, n, cap, batch, s);
                break;
            case ET_BF16:
                rc = launch_weight_grad_typed<__bf16, float>(vec, pack, n, cap, batch, s);
                break;
            default:  // ET_F16
                rc = launch_weight_grad_typed<_Float16, float>(vec, pack, n, cap, batch, s);
        }
        if (rc != ET_OK) return rc;
    }
    return ET_OK;
}
