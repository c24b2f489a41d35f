// et_weighted_update.hip — sparse SGD over weighted ragged gradients (et_weighted_sgd),
// textually included by et_update.hip after et_ragged_update.hip: the front of the pipeline
// is et_ragged_sgd's unchanged (group_occurrences over the values as a vector index, then
// k_ragged_bag_ids).  What is new is that every entry's gradient column is scaled by the
// entry's weight before it is added.
//
// Semantics (include/embtab.h): for every distinct column, acc = +0; for its participating
// entries in increasing k, t = C(w_k) * C(delta[:, bag(k)]), acc = acc + t (two roundings);
// then the update of sgd_apply_t.  Entries of the capacity tail (bag id 0) contribute nothing
// and their weights are never read; a column with no participating entry is not written.
// Never split: a hot column is one serial chain on one wave, as in et_ragged_sgd.

namespace et {

struct WeightPtrs {
    const void* w[ET_MAX_TABLES_PER_LAUNCH];
};

// k_ragged_apply with a weight per entry.  The lane that fetches an entry's bag id also
// fetches its weight: the entry id in `vals` is global, table t's weights start at occ_off[t].
template <typename T, typename C, int MODE, bool NT>
__global__ __launch_bounds__(256) void k_weighted_apply(
    UpdatePack pack, WeightPtrs wts, int ntables, const uint32_t* __restrict__ keys,
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
        const C* __restrict__ wt = reinterpret_cast<const C*>(wts.w[t]);
        const uint32_t occ = pack.occ_off[t];
        const uint64_t ldd = (uint64_t)d.ld_delta;
        T* w = col_ptr<T>(d.table, d.ld_table, d.cols_per_page, (uint64_t)(key - pack.row_off[t]));
        for (int f0 = 0; f0 < dim; f0 += 64 * K) {
            C acc[K];
#pragma unroll
            for (int k = 0; k < K; ++k) acc[k] = C(0);
            bool any = false;
            for (uint32_t e0 = ss; e0 < se; e0 += 64) {
                // the bags and weights of the next 64 entries, one per lane, handed out with
                // a shuffle; an entry without a bag (the capacity tail) reads no weight
                const uint32_t cnt = se - e0 < 64u ? se - e0 : 64u;
                const uint32_t mye = (uint32_t)lane < cnt ? vals[e0 + lane] : 0u;
                const uint32_t myb = (uint32_t)lane < cnt ? bag_ids[mye] : 0u;
                const C myw = myb != 0u ? wt[mye - occ] : C(0);
                for (uint32_t j0 = 0; j0 < cnt; j0 += E) {
                    uint32_t b[E];  // 0 beyond the segment (lanes >= cnt hold 0)
                    C wk[E];
#pragma unroll
                    for (int j = 0; j < E; ++j) {
                        b[j] = (uint32_t)__shfl((int)myb, (int)(j0 + j), 64);
                        wk[j] = __shfl(myw, (int)(j0 + j), 64);
                    }
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
                        for (int k = 0; k < K; ++k) {
                            const C tk = wk[j] * C(x[j][k]);
                            acc[k] = acc[k] + tk;
                        }
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

// The descriptors as et_ragged_update_desc (the shared front validates and sizes those).
inline void weighted_as_ragged(const et_weighted_update_desc* descs, int ntables,
                               et_ragged_update_desc* out) {
    for (int t = 0; t < ntables; ++t) {
        const et_weighted_update_desc& d = descs[t];
        out[t] = et_ragged_update_desc{d.table,  d.ld_table, d.nrows, d.dim,   0, d.delta,
                                       d.ld_delta, d.idx,    d.nnz,   d.colptr, d.batch,
                                       d.cols_per_page};
    }
}

inline int validate_weighted_update(const et_weighted_update_desc* descs, int ntables,
                                    et_ragged_update_desc* rd, int64_t* n_out, bool need_ptrs) {
    if (ntables < 0) return fail(ET_ERR_ARG, "negative ntables");
    if (ntables > ET_MAX_TABLES_PER_LAUNCH)
        return fail(ET_ERR_ARG, "at most %d tables per update call", ET_MAX_TABLES_PER_LAUNCH);
    if (ntables > 0 && !descs) return fail(ET_ERR_ARG, "descs is NULL");
    weighted_as_ragged(descs, ntables, rd);
    return validate_ragged_update(rd, ntables, n_out, need_ptrs);
}

}  // namespace et

extern "C" int et_weighted_sgd_workspace_size(const et_weighted_update_desc* descs,
                                              int32_t ntables, int64_t* bytes) {
    et::clear_err();
    if (!bytes) return et::fail(ET_ERR_ARG, "bytes is NULL");
    et_ragged_update_desc rd[ET_MAX_TABLES_PER_LAUNCH];
    int64_t n;
    const int rc = et::validate_weighted_update(descs, ntables, rd, &n, false);
    if (rc != ET_OK) return rc;
    *bytes = et::carve_ragged_ws(nullptr, n).bytes;
    return ET_OK;
}

extern "C" int et_weighted_sgd(int dtype, const et_weighted_update_desc* descs, int32_t ntables,
                               double eta, uint32_t flags, void* workspace, int64_t ws_bytes,
                               void* stream) {
    et::clear_err();
    et::open_side_streams(static_cast<hipStream_t>(stream));  // queue order only: none is used
    if (dtype != ET_F32 && dtype != ET_F64 && dtype != ET_F16 && dtype != ET_BF16)
        return et::fail(ET_ERR_UNSUPPORTED, "weighted SGD: dtype %d", dtype);
    if (flags & (ET_FLAG_SGD_INDEX_ONLY | ET_FLAG_SGD_APPLY_ONLY | ET_FLAG_SGD_HOT_PASS))
        return et::fail(ET_ERR_UNSUPPORTED,
                        "weighted SGD has no phased form and no hot-column pass");
    et_ragged_update_desc rd[ET_MAX_TABLES_PER_LAUNCH];
    int64_t n;
    int rc = et::validate_weighted_update(descs, ntables, rd, &n, true);
    if (rc != ET_OK) return rc;
    const int wsz = dtype == ET_F64 ? 8 : 4;
    for (int t = 0; t < ntables; ++t) {
        const et_weighted_update_desc& d = descs[t];
        if (d.nnz == 0 || d.batch == 0 || d.dim == 0) continue;
        if (!d.weights) return et::fail(ET_ERR_ARG, "table %d: NULL weights", t);
        if (reinterpret_cast<uintptr_t>(d.weights) % wsz != 0)
            return et::fail(ET_ERR_ARG, "table %d: weights not aligned to their element type", t);
    }
    if (n == 0) return ET_OK;
    et::RaggedWs w = et::carve_ragged_ws(static_cast<char*>(workspace), n);
    if (!workspace || ws_bytes < w.bytes)
        return et::fail(ET_ERR_WORKSPACE, "workspace of %lld bytes needed", (long long)w.bytes);
    hipStream_t s = static_cast<hipStream_t>(stream);

    // the values as a vector index: pool = 1, one "bag" per entry (as et_ragged_sgd)
    et::UpdatePack pack;
    et::RaggedBagArgs ba{};
    et::WeightPtrs wts{};
    uint32_t ro = 0, oo = 0;
    int64_t max_batch = 0;
    pack.vec_mask = 0;
    for (int t = 0; t < ntables; ++t) {
        const et_ragged_update_desc& r = rd[t];
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
        wts.w[t] = descs[t].weights;
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

    // Float16 sums in Float32: ET_FLAG_F16_FP32_ACC is implied
    const double eta_c = et::convert_eta(dtype, eta);
    const int64_t nb = et::cdiv64(n, 4);
    const unsigned grid = (unsigned)(nb < 16384 ? nb : 16384);
    return et::dispatch_sgd(dtype, flags | ET_FLAG_F16_FP32_ACC, [&](auto e, auto mode, auto nt) {
        using T = typename decltype(e)::type;
        using C = typename decltype(e)::acc;
        if constexpr (sizeof(C) == 2) {  // never selected: the flag above picks Float32 sums
            return et::fail(ET_ERR_UNSUPPORTED, "weighted SGD sums Float16 in Float32");
        } else {
        hipLaunchKernelGGL(
            (et::k_weighted_apply<T, C, decltype(mode)::value, decltype(nt)::value>), dim3(grid),
            dim3(256), 0, s, pack, wts, ntables, gr.keys, gr.vals, w.u.seg_start, w.u.counters,
            w.bag, sent, (C)eta_c, eta);
        ET_LAUNCH_CHECK("k_weighted_apply");
        return (int)ET_OK;
        }
    });
}
