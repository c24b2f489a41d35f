// et_ragged.hip — pooled lookup over variable-length bags (values + colptr), textually
// included by et_lookup.hip inside namespace et: it reuses VecGeom, idx_row32, pack16 /
// unpack16, col_ptr, the store helpers and note_oob of that translation unit.
//
// The reference has no ragged form; the semantics extend its pooled sum
// (src/lookup.jl:134-147): a bag's result is a COPY of its first row, then the remaining
// rows are added one at a time in index order, so a bag of length L equals the fixed-pool
// kernels' result for pool = L bit for bit.  An empty bag writes zero(T).
//
// Geometry (the fixed-pool vector kernel's, DESIGN.md §Ragged bags): the LPR lanes of a lane
// group own one row as 16-byte pieces, a wave holds GPW bags, U rows per group are issued
// before the first is consumed.  What differs is that the bags of one wave have different
// lengths: each group reads its own two colptr entries, clamps them, and walks [lo, hi);
// the groups of a wave run under the exec mask until the longest is done.  Because the
// groups' loop counters differ, an index is handed from the lane that loaded it to its
// group with ds_bpermute (a per-lane source), never v_readlane (a wave-uniform one).  No
// LDS allocation, no barriers.
//
// No wild reads: lo = colptr[j] - 1 and hi = colptr[j+1] - 1 are clamped to
// 0 <= lo <= hi <= nnz before anything is read through them (nnz is the capacity of the
// values buffer); each bound that needed clamping counts one out-of-range event.

struct RaggedPack {
    et_ragged_desc d[ET_MAX_TABLES_PER_LAUNCH];
};

// UU rows of one bag: slots i0 .. i0+UU-1 of the group's current index chunk (all valid;
// `myr` is the idx_row32 of the index this lane loaded).  Every load is issued before the
// first add, then the rows are added in slot order.  i0 may differ between the groups of a
// wave, hence the per-lane shuffle.  `paged`: table is an array of page pointers.
template <typename T, typename A, int D, int UU>
__device__ __forceinline__ void ragged_load_add(const T* __restrict__ table, uint32_t ld_table,
                                                uint32_t cpp, uint32_t myr, int gbase, int sub,
                                                int i0, bool first,
                                                A (&acc)[VecGeom<T, D>::NV][VecGeom<T, D>::N],
                                                int& bad, int vpr) {
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
                if (u == 0)
                    acc[v][k] = first ? A(x[k]) : A(acc[v][k] + A(x[k]));
                else
                    acc[v][k] = A(acc[v][k] + A(x[k]));
            }
        }
    }
}

// Ragged pooled sum, vector path: any row that is a multiple of 16 bytes, at the
// power-of-two capacity D of its dim (lanes beyond the row are masked).  Grid =
// ntables * ceil(batch / (4 * GPW)) workgroups of 256, tables interleaved as k_pooled_vec.
template <typename T, typename A, int D>
__global__ __launch_bounds__(256) void k_ragged_vec(RaggedPack pack, int ntables, int64_t batch,
                                                    T* __restrict__ dst, int64_t ld_dst, int nt) {
    using G = VecGeom<T, D>;
    constexpr int N = G::N, LPR = G::LPR, NV = G::NV, U = G::U;
    const int64_t item = blockIdx.x;
    const int t = (int)(item % ntables);
    const int64_t chunk = item / ntables;
    const et_ragged_desc& d = pack.d[t];
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
    const int64_t len = hi - lo;

    A acc[NV][N];
#pragma unroll
    for (int v = 0; v < NV; ++v)
#pragma unroll
        for (int k = 0; k < N; ++k) acc[v][k] = A(0);

    for (int64_t c0 = 0; c0 < len; c0 += LPR) {
        const int cnt = len - c0 < LPR ? (int)(len - c0) : LPR;
        // one 8-byte index per lane (a bag starts at any 8-byte boundary); lanes past the
        // end re-read the last one
        const uint32_t myr = idx_row32((long long)ip[c0 + (sub < cnt ? sub : cnt - 1)], nr);
        int i0 = 0;
#define ET_RG_LOAD_ADD(UU)                                                                     \
    ragged_load_add<T, A, D, UU>(table, ldt, cpp, myr, gbase, sub, i0, c0 == 0 && i0 == 0, acc, \
                                 bad, vpr)
        for (; i0 + U <= cnt; i0 += U) ET_RG_LOAD_ADD(U);
        if constexpr (U > 4) {
            if (cnt - i0 >= 4) {
                ET_RG_LOAD_ADD(4);
                i0 += 4;
            }
        }
        if constexpr (U > 2) {
            if (cnt - i0 >= 2) {
                ET_RG_LOAD_ADD(2);
                i0 += 2;
            }
        }
        if constexpr (U > 1) {
            if (cnt - i0 >= 1) ET_RG_LOAD_ADD(1);
        }
#undef ET_RG_LOAD_ADD
    }
    if (bad && sub == 0) note_oob(bad);
    u32x4* o = reinterpret_cast<u32x4*>(dst + bag * ld_dst + d.dst_row_off) + sub;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        T y[N];
#pragma unroll
        for (int k = 0; k < N; ++k) y[k] = T(acc[v][k]);
        if (sub + v * LPR < vpr) {
            if (nt)
                store16<true>(o + v * LPR, pack16<T, N>(y));
            else
                store16<false>(o + v * LPR, pack16<T, N>(y));
        }
    }
}

// Generic path (modelled on k_pooled_generic): any dim / alignment / element type, paged
// and column-pointer tables through col_ptr.  One wave per bag, lanes stride over the
// features, the bag's entries sequential per feature.
template <typename T, typename A>
__global__ __launch_bounds__(256) void k_ragged_generic(RaggedPack pack, int ntables,
                                                        int64_t batch, T* __restrict__ dst,
                                                        int64_t ld_dst, int nt) {
    constexpr int K = 4;
    const int64_t item = blockIdx.x;
    const int t = (int)(item % ntables);
    const int64_t chunk = item / ntables;
    const et_ragged_desc& d = pack.d[t];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t bag = chunk * 4 + wave;
    if (bag >= batch) return;
    int64_t lo, hi;
    int clamped;
    ragged_range(d.colptr, bag, d.nnz, lo, hi, clamped);
    if (clamped && lane == 0) note_oob(clamped);
    T* out = dst + bag * ld_dst + d.dst_row_off;
    const int dim = d.dim;
    for (int f0 = 0; f0 < dim; f0 += 64 * K) {
        A acc[K];
#pragma unroll
        for (int k = 0; k < K; ++k) acc[k] = A(0);
        for (int64_t i = lo; i < hi; ++i) {
            uint64_t row = (uint64_t)(d.idx[i] - 1);
            const bool ok = row < (uint64_t)d.nrows;
            if (!ok && lane == 0 && f0 == 0) note_oob();
            row = ok ? row : 0;
            const T* src = col_ptr<const T>(d.table, d.ld_table, d.cols_per_page, row);
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const int f = f0 + lane + 64 * k;
                if (f < dim) {
                    const T x = ok ? src[f] : T(0);
                    acc[k] = i == lo ? A(x) : A(acc[k] + A(x));
                }
            }
        }
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int f = f0 + lane + 64 * k;
            if (f < dim) {
                if (nt)
                    store_scalar<true>(out + f, T(acc[k]));
                else
                    store_scalar<false>(out + f, T(acc[k]));
            }
        }
    }
}

// ---------------------------------------------------------------------------
// Host dispatch
// ---------------------------------------------------------------------------

template <typename T, typename A, int D>
int launch_ragged_vec_d(const RaggedPack& pack, int n, int64_t batch, void* dst, int64_t ld_dst,
                        bool nt, hipStream_t s) {
    const int64_t per = 4 * VecGeom<T, D>::GPW;
    const int64_t grid = (batch + per - 1) / per * n;
    if (grid > 0x7fffffffll) return fail(ET_ERR_ARG, "grid too large");
    hipLaunchKernelGGL((k_ragged_vec<T, A, D>), dim3((unsigned)grid), dim3(256), 0, s, pack, n,
                       batch, reinterpret_cast<T*>(dst), ld_dst, nt ? 1 : 0);
    ET_LAUNCH_CHECK("k_ragged_vec");
    return ET_OK;
}

template <typename T, typename A>
int launch_ragged_vec(const RaggedPack& pack, int n, int D, int64_t batch, void* dst,
                      int64_t ld_dst, bool nt, hipStream_t s) {
#define ET_RG(C)                                                                       \
    case C:                                                                            \
        if constexpr (C / (16 / (int)sizeof(T)) >= 1)                                  \
            return launch_ragged_vec_d<T, A, C>(pack, n, batch, dst, ld_dst, nt, s);   \
        break;
    switch (masked_capacity(D)) {
        ET_RG(16)
        ET_RG(32)
        ET_RG(64)
        ET_RG(128)
        ET_RG(256)
        ET_RG(512)
        ET_RG(1024)
        ET_RG(2048)
    }
#undef ET_RG
    return fail(ET_ERR_UNSUPPORTED, "ragged vector dim %d", D);
}

template <typename T, typename A>
int launch_ragged_typed(bool vec, const RaggedPack& pack, int n, int D, int64_t batch, void* dst,
                        int64_t ld_dst, bool nt, hipStream_t s) {
    if (vec) return launch_ragged_vec<T, A>(pack, n, D, batch, dst, ld_dst, nt, s);
    const int64_t grid = (batch + 3) / 4 * n;
    if (grid > 0x7fffffffll) return fail(ET_ERR_ARG, "grid too large");
    hipLaunchKernelGGL((k_ragged_generic<T, A>), dim3((unsigned)grid), dim3(256), 0, s, pack, n,
                       batch, reinterpret_cast<T*>(dst), ld_dst, nt ? 1 : 0);
    ET_LAUNCH_CHECK("k_ragged_generic");
    return ET_OK;
}

inline int launch_ragged_group(int dtype, bool f32acc, bool vec, const RaggedPack& pack, int n,
                               int D, int64_t batch, void* dst, int64_t ld_dst, bool nt,
                               hipStream_t s) {
    switch (dtype) {
        case ET_F32:
            return launch_ragged_typed<float, float>(vec, pack, n, D, batch, dst, ld_dst, nt, s);
        case ET_F64:
            return launch_ragged_typed<double, double>(vec, pack, n, D, batch, dst, ld_dst, nt, s);
        case ET_I32:
            return launch_ragged_typed<int32_t, uint32_t>(vec, pack, n, D, batch, dst, ld_dst, nt,
                                                          s);
        case ET_I64:
            return launch_ragged_typed<int64_t, uint64_t>(vec, pack, n, D, batch, dst, ld_dst, nt,
                                                          s);
        case ET_BF16:  // fp32 accumulation, one RNE rounding per output element
            return launch_ragged_typed<__bf16, float>(vec, pack, n, D, batch, dst, ld_dst, nt, s);
        case ET_F16:
            if (f32acc)
                return launch_ragged_typed<_Float16, float>(vec, pack, n, D, batch, dst, ld_dst,
                                                            nt, s);
            return launch_ragged_typed<_Float16, _Float16>(vec, pack, n, D, batch, dst, ld_dst, nt,
                                                           s);
    }
    return fail(ET_ERR_UNSUPPORTED, "dtype %d", dtype);
}

// Validate, group the tables by (kernel, dim) and launch one kernel per group.
inline int ragged_dispatch(int dtype, const et_ragged_desc* descs, int ntables, int64_t batch,
                           void* dst, int64_t ld_dst, uint32_t flags, hipStream_t s) {
    const int es = elsize(dtype);
    if (es == 0) return fail(ET_ERR_UNSUPPORTED, "unknown dtype %d", dtype);
    if (ntables < 0 || batch < 0) return fail(ET_ERR_ARG, "negative ntables/batch");
    if (ntables > ET_MAX_TABLES_PER_LAUNCH)
        return fail(ET_ERR_ARG, "at most %d tables per ragged lookup", ET_MAX_TABLES_PER_LAUNCH);
    if (ntables == 0 || batch == 0) return ET_OK;
    if (batch >= 0x7fffffffll) return fail(ET_ERR_ARG, "batch too large");
    if (!descs) return fail(ET_ERR_ARG, "descs is NULL");
    if (!dst) return fail(ET_ERR_ARG, "dst is NULL");
    int kind_of[ET_MAX_TABLES_PER_LAUNCH];  // -1 nothing, 0 generic, 1 vector
    for (int t = 0; t < ntables; ++t) {
        const et_ragged_desc& d = descs[t];
        if (d.dim < 0 || d.nrows < 0 || d.nnz < 0 || d.cols_per_page < 0)
            return fail(ET_ERR_ARG, "table %d: negative dim/nrows/nnz/cols_per_page", t);
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
        const bool al = ((d.ld_table * es) % 16 == 0) && ((int64_t)d.dim * es) % 16 == 0 &&
                        (d.cols_per_page > 0 || aligned16(d.table)) &&
                        aligned16(static_cast<char*>(dst) + d.dst_row_off * es) &&
                        ((ld_dst * es) % 16 == 0);
        const bool vec = al && d.dim <= 2048 && d.nnz > 0 && d.nrows < 0xffffffffll &&
                         d.ld_table < 0xffffffffll && d.cols_per_page < 0xffffffffll;
        kind_of[t] = vec ? 1 : 0;
    }
    const bool nt = (flags & ET_FLAG_NONTEMPORAL) != 0;
    const bool f32acc = (flags & ET_FLAG_F16_FP32_ACC) != 0;
    bool done[ET_MAX_TABLES_PER_LAUNCH] = {false};
    for (int t0 = 0; t0 < ntables; ++t0) {
        if (done[t0] || kind_of[t0] < 0) continue;
        RaggedPack pack;
        int n = 0;
        const bool vec = kind_of[t0] == 1;
        // vector groups share a capacity (the kernel reads each table's own dim)
        const int cap = vec ? masked_capacity(descs[t0].dim) : 0;
        for (int t = t0; t < ntables; ++t) {
            if (done[t] || kind_of[t] != kind_of[t0]) continue;
            if (vec && masked_capacity(descs[t].dim) != cap) continue;
            pack.d[n++] = descs[t];
            done[t] = true;
        }
        const int rc = launch_ragged_group(dtype, f32acc, vec, pack, n, cap, batch, dst, ld_dst,
                                           nt, s);
        if (rc != ET_OK) return rc;
    }
    return ET_OK;
}
