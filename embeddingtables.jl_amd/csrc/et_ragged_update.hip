// et_ragged_update.hip — sparse SGD over ragged gradients (values + colptr) and the bag id
// of every entry, textually included by et_update.hip: the front of the pipeline is
// group_occurrences unchanged (keys, stable segmented radix sort, segments), run over the
// values as a vector index (pool = 1), which leaves per distinct (table, column) its entry
// ids in increasing order.  What is new is where an entry's gradient column comes from:
// its bag id (k_ragged_bag_ids) instead of occurrence / pool.
//
// Semantics (extending src/sparseupdate.jl:97-129, the serial per-column sum): for every
// distinct column, acc = +0, then delta[:, bag(k)] is added for each of its entries k in
// increasing k, then the update is sgd_apply_t.  Entries of the capacity tail (bag id 0)
// contribute nothing; a column with no participating entry is not written.  No column is
// ever split: a hot column is one serial chain on one wave (DESIGN.md §Ragged bags).

namespace et {

struct RaggedBagArgs {
    const int64_t* colptr[ET_MAX_TABLES_PER_LAUNCH];
    int64_t batch[ET_MAX_TABLES_PER_LAUNCH];
    int64_t nnz[ET_MAX_TABLES_PER_LAUNCH];
    int64_t off[ET_MAX_TABLES_PER_LAUNCH];  // first entry of table t in `out`
};

// out[off_t + k] = 1-based bag of entry k of table t = blockIdx.y: every bag writes its
// (clamped) range, 16 lanes per bag.  Entries no bag covers keep the 0 of the memset that
// precedes the launch.
template <typename O>
__global__ __launch_bounds__(256) void k_ragged_bag_ids(RaggedBagArgs a, O* __restrict__ out) {
    const int t = blockIdx.y;
    const int sub = threadIdx.x & 15;
    const int64_t batch = a.batch[t], nnz = a.nnz[t];
    const int64_t* __restrict__ colptr = a.colptr[t];
    O* __restrict__ o = out + a.off[t];
    for (int64_t bag = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4); bag < batch;
         bag += (int64_t)gridDim.x * 16) {
        int64_t lo, hi;
        int clamped;
        ragged_range(colptr, bag, nnz, lo, hi, clamped);
        if (clamped && sub == 0) note_oob(clamped);
        for (int64_t k = lo + sub; k < hi; k += 16) o[k] = (O)(bag + 1);
    }
}

template <typename O>
int launch_ragged_bag_ids(const RaggedBagArgs& a, int ntables, int64_t max_batch, O* out,
                          hipStream_t s) {
    if (ntables <= 0 || max_batch <= 0) return ET_OK;
    const int64_t nb = cdiv64(max_batch, 16);
    hipLaunchKernelGGL((k_ragged_bag_ids<O>), dim3((unsigned)(nb < 16384 ? nb : 16384), ntables),
                       dim3(256), 0, s, a, out);
    ET_LAUNCH_CHECK("k_ragged_bag_ids");
    return ET_OK;
}

// One wave per segment (distinct table column): walk its entries in increasing entry id,
// eight gradient rows in flight, add them in order, apply the update.  T the table's
// element type, C the accumulator (sgd_apply_t).
template <typename T, typename C, int MODE, bool NT>
__global__ __launch_bounds__(256) void k_ragged_apply(
    UpdatePack pack, int ntables, const uint32_t* __restrict__ keys,
    const uint32_t* __restrict__ vals, const uint32_t* __restrict__ seg_start,
    const uint32_t* __restrict__ counters, const uint32_t* __restrict__ bag_ids, uint32_t sent,
    C eta_c, double eta64) {
    constexpr int K = 4, E = 8;  // E divides 64
    const int lane = threadIdx.x & 63;
    const uint32_t U = counters[kCntU];
    for (uint32_t u = blockIdx.x * 4 + (threadIdx.x >> 6); u < U; u += gridDim.x * 4) {
        const uint32_t ss = seg_start[u], se = seg_start[u + 1], key = keys[ss];
        if (key >= sent) continue;  // out-of-range indices (counted by the key pass)
        const int t = table_of_key(pack, ntables, key);
        const et_update_desc& d = pack.d[t];
        const int dim = d.dim;
        const T* __restrict__ delta = reinterpret_cast<const T*>(d.delta);
        const uint64_t ldd = (uint64_t)d.ld_delta;
        T* w = col_ptr<T>(d.table, d.ld_table, d.cols_per_page, (uint64_t)(key - pack.row_off[t]));
        for (int f0 = 0; f0 < dim; f0 += 64 * K) {
            C acc[K];
#pragma unroll
            for (int k = 0; k < K; ++k) acc[k] = C(0);
            bool any = false;
            for (uint32_t e0 = ss; e0 < se; e0 += 64) {
                // the bags of the next 64 entries, one per lane (two dependent loads per 64
                // entries instead of per entry), handed out with a shuffle
                const uint32_t cnt = se - e0 < 64u ? se - e0 : 64u;
                const uint32_t myb = (uint32_t)lane < cnt ? bag_ids[vals[e0 + lane]] : 0u;
                for (uint32_t j0 = 0; j0 < cnt; j0 += E) {
                    uint32_t b[E];  // 0 beyond the segment (lanes >= cnt hold 0)
#pragma unroll
                    for (int j = 0; j < E; ++j)
                        b[j] = (uint32_t)__shfl((int)myb, (int)(j0 + j), 64);
                    T x[E][K];
#pragma unroll
                    for (int j = 0; j < E; ++j)
#pragma unroll
                        for (int k = 0; k < K; ++k) {
                            const int f = f0 + lane + 64 * k;
                            x[j][k] = b[j] != 0u && f < dim
                                          ? delta[(uint64_t)(b[j] - 1u) * ldd + f]
                                          : T(0);
                        }
#pragma unroll
                    for (int j = 0; j < E; ++j) {
                        if (b[j] == 0u) continue;  // capacity tail: no bag, nothing added
                        any = true;
#pragma unroll
                        for (int k = 0; k < K; ++k) acc[k] = acc[k] + C(x[j][k]);
                    }
                }
            }
            if (!any) break;  // no participating entry: the column is not written
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const int f = f0 + lane + 64 * k;
                if (f < dim)
                    store_scalar<NT>(w + f, sgd_apply_t<T, C, MODE>(w[f], acc[k], eta_c, eta64));
            }
        }
    }
}

struct RaggedWs {
    UpdateWs u;
    uint32_t* bag;  // bag id of every entry, tables back to back
    int64_t bytes;
};

inline RaggedWs carve_ragged_ws(char* base, int64_t n) {
    RaggedWs w;
    w.u = plan_index_ws(base, n);
    w.bag = base ? reinterpret_cast<uint32_t*>(base + w.u.bytes) : nullptr;
    w.bytes = w.u.bytes + align256(4 * (n + 1));
    return w;
}

// Descriptor checks; *n_out = entries of all tables with work (a table with no bags or no
// features has none).
inline int validate_ragged_update(const et_ragged_update_desc* descs, int ntables,
                                  int64_t* n_out, bool need_ptrs) {
    if (ntables < 0) return fail(ET_ERR_ARG, "negative ntables");
    if (ntables > ET_MAX_TABLES_PER_LAUNCH)
        return fail(ET_ERR_ARG, "at most %d tables per update call", ET_MAX_TABLES_PER_LAUNCH);
    if (ntables > 0 && !descs) return fail(ET_ERR_ARG, "descs is NULL");
    int64_t n = 0;
    uint64_t rows = 0;
    for (int t = 0; t < ntables; ++t) {
        const et_ragged_update_desc& d = descs[t];
        if (d.dim < 0 || d.nrows < 0 || d.nnz < 0 || d.batch < 0 || d.cols_per_page < 0)
            return fail(ET_ERR_ARG, "table %d: negative size", t);
        if (d.batch >= 0xffffffffll) return fail(ET_ERR_ARG, "table %d: batch too large", t);
        rows += (uint64_t)d.nrows;
        if (d.nnz == 0 || d.batch == 0 || d.dim == 0) continue;
        if (need_ptrs && (!d.idx || !d.colptr || !d.table || !d.delta))
            return fail(ET_ERR_ARG, "table %d: NULL", t);
        if (d.ld_table < d.dim || d.ld_delta < d.dim)
            return fail(ET_ERR_ARG, "table %d: leading dimension < dim", t);
        n += d.nnz;
        if (n >= 0x7fffffffll) return fail(ET_ERR_ARG, "too many entries");
    }
    if (rows >= 0xffffffffull) return fail(ET_ERR_ARG, "too many table columns");
    *n_out = n;
    return ET_OK;
}

}  // namespace et

extern "C" int et_ragged_bag_ids(const int64_t* colptr, int64_t batch, int64_t nnz, int64_t* bag,
                                 void* stream) {
    et::clear_err();
    if (batch < 0 || nnz < 0) return et::fail(ET_ERR_ARG, "negative size");
    if (nnz == 0) return ET_OK;
    if (!bag) return et::fail(ET_ERR_ARG, "bag is NULL");
    if (batch > 0 && !colptr) return et::fail(ET_ERR_ARG, "colptr is NULL");
    hipStream_t s = static_cast<hipStream_t>(stream);
    ET_HIP_CHECK(hipMemsetAsync(bag, 0, (size_t)nnz * 8, s));
    et::RaggedBagArgs a{};
    a.colptr[0] = colptr;
    a.batch[0] = batch;
    a.nnz[0] = nnz;
    a.off[0] = 0;
    return et::launch_ragged_bag_ids<int64_t>(a, 1, batch, bag, s);
}

extern "C" int et_ragged_sgd_workspace_size(const et_ragged_update_desc* descs, int32_t ntables,
                                            int64_t* bytes) {
    et::clear_err();
    if (!bytes) return et::fail(ET_ERR_ARG, "bytes is NULL");
    int64_t n;
    const int rc = et::validate_ragged_update(descs, ntables, &n, false);
    if (rc != ET_OK) return rc;
    *bytes = et::carve_ragged_ws(nullptr, n).bytes;
    return ET_OK;
}

extern "C" int et_ragged_sgd(int dtype, const et_ragged_update_desc* descs, int32_t ntables,
                             double eta, uint32_t flags, void* workspace, int64_t ws_bytes,
                             void* stream) {
    et::clear_err();
    et::open_side_streams(static_cast<hipStream_t>(stream));  // queue order only: none is used
    if (dtype != ET_F32 && dtype != ET_F64 && dtype != ET_F16 && dtype != ET_BF16)
        return et::fail(ET_ERR_UNSUPPORTED, "ragged SGD: dtype %d", dtype);
    if (flags & (ET_FLAG_SGD_INDEX_ONLY | ET_FLAG_SGD_APPLY_ONLY | ET_FLAG_SGD_HOT_PASS))
        return et::fail(ET_ERR_UNSUPPORTED,
                        "ragged SGD has no phased form and no hot-column pass");
    int64_t n;
    int rc = et::validate_ragged_update(descs, ntables, &n, true);
    if (rc != ET_OK) return rc;
    if (n == 0) return ET_OK;
    et::RaggedWs w = et::carve_ragged_ws(static_cast<char*>(workspace), n);
    if (!workspace || ws_bytes < w.bytes)
        return et::fail(ET_ERR_WORKSPACE, "workspace of %lld bytes needed", (long long)w.bytes);
    hipStream_t s = static_cast<hipStream_t>(stream);

    // the values as a vector index: pool = 1, one "bag" per entry
    et::UpdatePack pack;
    et::RaggedBagArgs ba{};
    uint32_t ro = 0, oo = 0;
    int64_t max_batch = 0;
    pack.vec_mask = 0;
    for (int t = 0; t < ntables; ++t) {
        const et_ragged_update_desc& r = descs[t];
        const bool work = r.nnz > 0 && r.batch > 0 && r.dim > 0;
        et_update_desc d{};
        d.table = r.table;
        d.ld_table = r.ld_table;
        d.nrows = r.nrows;
        d.dim = r.dim;
        d.pool = 1;
        d.delta = r.delta;
        d.ld_delta = r.ld_delta;
        d.idx = r.idx;
        d.ld_idx = 1;
        d.batch = work ? r.nnz : 0;
        d.cols_per_page = r.cols_per_page;
        pack.d[t] = d;
        pack.row_off[t] = ro;
        pack.occ_off[t] = oo;
        ba.colptr[t] = r.colptr;
        ba.batch[t] = work ? r.batch : 0;
        ba.nnz[t] = work ? r.nnz : 0;
        ba.off[t] = (int64_t)oo;
        if (work && r.batch > max_batch) max_batch = r.batch;
        ro += (uint32_t)r.nrows;
        oo += (uint32_t)d.batch;
    }
    pack.row_off[ntables] = ro;
    pack.occ_off[ntables] = oo;
    const uint32_t sent = ro;  // key of out-of-range indices (sorts last)

    ET_HIP_CHECK(hipMemsetAsync(w.bag, 0, (size_t)n * 4, s));
    rc = et::launch_ragged_bag_ids<uint32_t>(ba, ntables, max_batch, w.bag, s);
    if (rc != ET_OK) return rc;
    et::Grouped gr;
    rc = et::group_occurrences(pack, ntables, n, sent, et::kChunk, w.u, gr, s);
    if (rc != ET_OK) return rc;

    const double eta_c = et::convert_eta(dtype, eta);
    const int64_t nb = et::cdiv64(n, 4);
    const unsigned grid = (unsigned)(nb < 16384 ? nb : 16384);
    return et::dispatch_sgd(dtype, flags, [&](auto e, auto mode, auto nt) {
        using T = typename decltype(e)::type;
        using C = typename decltype(e)::acc;
        hipLaunchKernelGGL((et::k_ragged_apply<T, C, decltype(mode)::value, decltype(nt)::value>),
                           dim3(grid), dim3(256), 0, s, pack, ntables, gr.keys, gr.vals,
                           w.u.seg_start, w.u.counters, w.bag, sent, (C)eta_c, eta);
        ET_LAUNCH_CHECK("k_ragged_apply");
        return (int)ET_OK;
    });
}
