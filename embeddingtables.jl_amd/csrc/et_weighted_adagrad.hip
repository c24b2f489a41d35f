// et_weighted_adagrad.hip — sparse AdaGrad over gradients that carry a weight per entry
// (et_weighted_adagrad), textually included by et_update.hip after et_adagrad.hip.  The front
// of the pipeline (prepare_adagrad: k_ragged_bag_ids, group_occurrences with chunk = kChunk),
// the combine kernels and the apply step are et_sparse_adagrad's, unchanged: only the chunk
// pass differs, by one multiply per element in front of the add.  The chunk kernels here are
// functions of their own, so the ones et_sparse_adagrad launches keep their code.
//
// Semantics (include/embtab.h): per chunk p_c = +0, then for every entry of the chunk that a
// bag covers t = C(w_k) * C(delta[:, bag(k)]), p_c = p_c + t (two roundings, never an fma);
// g = p_0, or ((p_0 + p_1) + p_2) + ... in chunk order.  An entry no bag covers adds nothing,
// keeps its list position, and its weight is never read.
//
// Where the weights ride: the chunk kernels get a copy of the UpdatePack whose d[t].idx holds
// table t's weights (NULL: a table without weights, every entry counts 1).  The key pass is
// the last reader of idx (the chunk pass reads the sorted occurrence ids), so the kernels'
// arguments stay the size of their unweighted twins', 32 tables and all.  The weight of sorted
// occurrence id o of table t is at o - occ_off[t], as in k_weighted_apply.

namespace et {

template <typename C>
__device__ __forceinline__ const C* ada_weights(const et_update_desc& d) {
    return reinterpret_cast<const C*>(d.idx);
}

// ada_occ_sum with a weight per occurrence: the lane that turns an occurrence id into a
// gradient column also fetches its weight (only when a bag covers the entry) and hands both
// out in the same shuffle step; each gathered row is multiplied before it is added.
template <int D, int U>
__device__ __forceinline__ bool ada_occ_wsum(const float* __restrict__ delta, uint64_t ldd,
                                             uint32_t occ_off, uint32_t pool, bool ragged,
                                             const float* __restrict__ wt,
                                             const uint32_t* __restrict__ bag_ids,
                                             const uint32_t* __restrict__ vals, uint32_t s0,
                                             uint32_t s1, int g, int sub, int vpr,
                                             float (&acc)[(D / 4 < 64 ? 1 : D / 4 / 64)][4]) {
    constexpr int VPR = D / 4;
    constexpr int LPR = VPR < 64 ? VPR : 64;
    constexpr int NV = VPR / LPR;
    int vix[NV];
    vec_index<LPR, NV>(sub, vpr, vix);
    bool any = false;
    for (uint32_t c0 = s0; c0 < s1; c0 += LPR) {
        const int cnt = (int)(s1 - c0 < (uint32_t)LPR ? s1 - c0 : (uint32_t)LPR);
        uint32_t myb = 0;
        float myw = 1.0f;
        if (sub < cnt) {
            const uint32_t o = vals[c0 + (uint32_t)sub];
            myb = ada_bag(o, ragged, occ_off, pool, bag_ids);
            if (wt != nullptr && myb != 0u) myw = wt[o - occ_off];
        }
        for (int i0 = 0; i0 < cnt; i0 += U) {
            uint32_t b[U];
            float wk[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int j = i0 + u;
                const int src = g * LPR + (j < LPR ? j : LPR - 1);
                const uint32_t v = (uint32_t)__shfl((int)myb, src, 64);
                wk[u] = __shfl(myw, src, 64);
                b[u] = j < cnt ? v : 0u;
            }
            u32x4 buf[U][NV];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const u32x4* src =
                    reinterpret_cast<const u32x4*>(delta + (uint64_t)(b[u] ? b[u] - 1u : 0u) * ldd);
#pragma unroll
                for (int v = 0; v < NV; ++v) buf[u][v] = b[u] ? src[vix[v]] : u32x4{0u, 0u, 0u, 0u};
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (b[u] == 0u) continue;  // past the chunk, or an entry no bag covers
                any = true;
#pragma unroll
                for (int v = 0; v < NV; ++v) {
                    const float t0 = wk[u] * __uint_as_float(buf[u][v].x);
                    const float t1 = wk[u] * __uint_as_float(buf[u][v].y);
                    const float t2 = wk[u] * __uint_as_float(buf[u][v].z);
                    const float t3 = wk[u] * __uint_as_float(buf[u][v].w);
                    acc[v][0] = acc[v][0] + t0;
                    acc[v][1] = acc[v][1] + t1;
                    acc[v][2] = acc[v][2] + t2;
                    acc[v][3] = acc[v][3] + t3;
                }
            }
        }
    }
    return any;
}

// k_adagrad_chunks with weights (pack.d[t].idx: see the head of this file).
template <int D, bool ROW, bool NT>
__global__ __launch_bounds__(256) void k_weighted_adagrad_chunks(
    UpdatePack pack, AdaPack ap, int ntables, const uint32_t* __restrict__ vals,
    const ChunkRec* __restrict__ recs, const uint32_t* __restrict__ counters,
    const uint32_t* __restrict__ bag_ids, float* __restrict__ partials,
    uint32_t* __restrict__ pany, int pdim, uint32_t sent, float eta, float eps,
    uint32_t my_mask) {
    constexpr int VPR = D / 4;
    constexpr int LPR = VPR < 64 ? VPR : 64;
    constexpr int NV = VPR / LPR;
    constexpr int GPW = 64 / LPR;
    constexpr int U = NV >= 8 ? 1 : 8 / NV;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = lane / LPR, sub = lane % LPR;
    const uint32_t Cn = counters[kCntC];
    const uint32_t ngroups = gridDim.x * 4u * GPW;
    for (uint32_t c = (blockIdx.x * 4u + wave) * GPW + g; c < Cn; c += ngroups) {
        const ChunkRec r = recs[c];
        if (r.key >= sent) continue;  // out-of-range indices (counted by the key pass)
        const int t = table_of_key(pack, ntables, r.key);
        if (!((my_mask >> t) & 1u)) continue;  // another capacity's / a generic table
        const et_update_desc& d = pack.d[t];
        const uint32_t row = r.key - pack.row_off[t];
        float* w = col_ptr<float>(d.table, d.ld_table, d.cols_per_page, row);
        float* sp = reinterpret_cast<float*>(ap.state[t]) +
                    (ROW ? (uint64_t)row : (uint64_t)row * (uint64_t)ap.ld_state[t]);
        const int vpr = d.dim / 4;
        int vix[NV];
        vec_index<LPR, NV>(sub, vpr, vix);
        const bool apply = r.dst == kApply;
        u32x4 x[NV], st[NV];
        float srow = 0.0f;
#pragma unroll
        for (int v = 0; v < NV; ++v) x[v] = st[v] = u32x4{0u, 0u, 0u, 0u};
        if (apply) {  // the column and its state first: their latency hides under the gathers
#pragma unroll
            for (int v = 0; v < NV; ++v) x[v] = reinterpret_cast<const u32x4*>(w)[vix[v]];
            if constexpr (ROW) {
                srow = *sp;
            } else {
#pragma unroll
                for (int v = 0; v < NV; ++v) st[v] = reinterpret_cast<const u32x4*>(sp)[vix[v]];
            }
        }
        float acc[NV][4];
#pragma unroll
        for (int v = 0; v < NV; ++v) acc[v][0] = acc[v][1] = acc[v][2] = acc[v][3] = 0.0f;
        const bool any = ada_occ_wsum<D, U>(
            reinterpret_cast<const float*>(d.delta), (uint64_t)d.ld_delta, pack.occ_off[t],
            (uint32_t)d.pool, (ap.ragged >> t) & 1u, ada_weights<float>(d), bag_ids, vals, r.s0,
            r.s1, g, sub, vpr, acc);
        if (apply) {
            if (any)  // no participating entry: neither the column nor its state is written
                ada_apply_row<D, ROW, NT>(w, sp, x, st, srow, acc, sub, vpr, d.dim, eta, eps);
        } else {
            u32x4* pp = reinterpret_cast<u32x4*>(partials + (uint64_t)r.dst * pdim) + sub;
#pragma unroll
            for (int v = 0; v < NV; ++v)
                if (sub + v * LPR < vpr)
                    pp[v * LPR] = u32x4{__float_as_uint(acc[v][0]), __float_as_uint(acc[v][1]),
                                        __float_as_uint(acc[v][2]), __float_as_uint(acc[v][3])};
            if (sub == 0) pany[r.dst] = any ? 1u : 0u;
        }
    }
}

// k_adagrad_chunks_generic with weights: every other element type, dim and alignment.
template <typename T, typename C, bool ROW, bool NT>
__global__ __launch_bounds__(256) void k_weighted_adagrad_chunks_generic(
    UpdatePack pack, AdaPack ap, int ntables, const uint32_t* __restrict__ vals,
    const ChunkRec* __restrict__ recs, const uint32_t* __restrict__ counters,
    const uint32_t* __restrict__ bag_ids, C* __restrict__ partials, uint32_t* __restrict__ pany,
    int pdim, uint32_t sent, C eta, C eps) {
    const int lane = threadIdx.x & 63;
    const uint32_t Cn = counters[kCntC];
    const uint32_t waves = gridDim.x * 4;
    for (uint32_t c = blockIdx.x * 4 + (threadIdx.x >> 6); c < Cn; c += waves) {
        const ChunkRec r = recs[c];
        if (r.key >= sent) continue;
        const int t = table_of_key(pack, ntables, r.key);
        if ((pack.vec_mask >> t) & 1u) continue;  // the vector kernels' table
        const et_update_desc& d = pack.d[t];
        const int dim = d.dim;
        const T* __restrict__ delta = reinterpret_cast<const T*>(d.delta);
        const C* __restrict__ wt = ada_weights<C>(d);
        const uint64_t ldd = (uint64_t)d.ld_delta;
        const bool ragged = (ap.ragged >> t) & 1u;
        const uint32_t occ_off = pack.occ_off[t], pool = (uint32_t)d.pool;
        const uint32_t s0 = r.s0, s1 = r.s1;
        auto sum_block = [&](int f0, C(&acc)[kAdaK]) -> bool {
#pragma unroll
            for (int k = 0; k < kAdaK; ++k) acc[k] = C(0);
            bool any = false;
            for (uint32_t e0 = s0; e0 < s1; e0 += 64) {
                const uint32_t cnt = s1 - e0 < 64u ? s1 - e0 : 64u;
                uint32_t myb = 0;
                C myw = C(1);
                if ((uint32_t)lane < cnt) {
                    const uint32_t o = vals[e0 + (uint32_t)lane];
                    myb = ada_bag(o, ragged, occ_off, pool, bag_ids);
                    if (wt != nullptr && myb != 0u) myw = wt[o - occ_off];
                }
                for (uint32_t j0 = 0; j0 < cnt; j0 += kAdaE) {
                    uint32_t b[kAdaE];  // 0 beyond the chunk (lanes >= cnt hold 0)
                    C wk[kAdaE];
#pragma unroll
                    for (int j = 0; j < kAdaE; ++j) {
                        b[j] = (uint32_t)__shfl((int)myb, (int)(j0 + j), 64);
                        wk[j] = __shfl(myw, (int)(j0 + j), 64);
                    }
                    T x[kAdaE][kAdaK];
#pragma unroll
                    for (int j = 0; j < kAdaE; ++j)
#pragma unroll
                        for (int k = 0; k < kAdaK; ++k) {
                            const int f = f0 + lane + 64 * k;
                            x[j][k] = b[j] != 0u && f < dim
                                          ? delta[(uint64_t)(b[j] - 1u) * ldd + f]
                                          : T(0);
                        }
#pragma unroll
                    for (int j = 0; j < kAdaE; ++j) {
                        if (b[j] == 0u) continue;
                        any = true;
#pragma unroll
                        for (int k = 0; k < kAdaK; ++k) {
                            const C tk = wk[j] * C(x[j][k]);
                            acc[k] = acc[k] + tk;
                        }
                    }
                }
            }
            return any;
        };
        if (r.dst != kApply) {
            C acc[kAdaK];
            bool any = false;
            for (int f0 = 0; f0 < dim; f0 += 64 * kAdaK) {
                any = sum_block(f0, acc);
#pragma unroll
                for (int k = 0; k < kAdaK; ++k) {
                    const int f = f0 + lane + 64 * k;
                    if (f < dim) partials[(uint64_t)r.dst * pdim + f] = acc[k];
                }
            }
            if (lane == 0) pany[r.dst] = any ? 1u : 0u;
            continue;
        }
        const uint32_t row = r.key - pack.row_off[t];
        T* w = col_ptr<T>(d.table, d.ld_table, d.cols_per_page, row);
        C* sp = reinterpret_cast<C*>(ap.state[t]) +
                (ROW ? (uint64_t)row : (uint64_t)row * (uint64_t)ap.ld_state[t]);
        ada_apply_generic<T, C, ROW, NT>(w, sp, dim, lane, eta, eps, sum_block);
    }
}

// launch_adagrad with the weighted chunk kernels; `wpack` is r.pack with the weights in idx.
// The combine kernels are et_sparse_adagrad's: the partial rows are already weighted.
template <typename T, typename C, bool ROW, bool NT>
int launch_weighted_adagrad(const AdaRun& r, const UpdatePack& wpack, C eta, C eps) {
    const unsigned grid = sgd_grid(r.n);
    const int64_t mmax = r.n / kChunk + 2;  // multi-chunk columns at most
    const UpdateWs& u = r.w.u;
    if constexpr (__is_same(T, float)) {
        float* partials = reinterpret_cast<float*>(r.w.partials);
        for (int i = 0; i < r.vg.n; ++i)
            with_capacity(r.vg.cap[i], [&](auto cap) {
                constexpr int D = decltype(cap)::value;
                constexpr int GPW = D / 4 < 64 ? 64 / (D / 4) : 1;
                const int64_t cb = cdiv64(mmax, 4 * GPW);
                hipLaunchKernelGGL((k_weighted_adagrad_chunks<D, ROW, NT>), dim3(grid), dim3(256),
                                   0, r.s, wpack, r.ap, r.ntables, r.gr.vals, u.recs, u.counters,
                                   r.w.bag, partials, r.w.pany, r.pdim, r.sent, eta, eps,
                                   r.vg.mask[i]);
                hipLaunchKernelGGL((k_adagrad_combine<D, ROW, NT>),
                                   dim3((unsigned)(cb < 2048 ? cb : 2048)), dim3(256), 0, r.s,
                                   r.pack, r.ap, r.ntables, r.gr.keys, u.seg_start, u.multi,
                                   u.counters, u.mlist, partials, r.w.pany, r.pdim, r.sent, eta,
                                   eps, r.vg.mask[i]);
            });
        ET_LAUNCH_CHECK("k_weighted_adagrad_chunks");
    }
    if (r.any_generic) {
        C* partials = reinterpret_cast<C*>(r.w.partials);
        const int64_t cb = cdiv64(mmax, 4);
        hipLaunchKernelGGL((k_weighted_adagrad_chunks_generic<T, C, ROW, NT>), dim3(grid),
                           dim3(256), 0, r.s, wpack, r.ap, r.ntables, r.gr.vals, u.recs,
                           u.counters, r.w.bag, partials, r.w.pany, r.pdim, r.sent, eta, eps);
        hipLaunchKernelGGL((k_adagrad_combine_generic<T, C, ROW, NT>),
                           dim3((unsigned)(cb < 4096 ? cb : 4096)), dim3(256), 0, r.s, r.pack, r.ap,
                           r.ntables, r.gr.keys, u.seg_start, u.multi, u.counters, u.mlist,
                           partials, r.w.pany, r.pdim, r.sent, eta, eps);
        ET_LAUNCH_CHECK("k_weighted_adagrad_chunks_generic");
    }
    return ET_OK;
}

// The descriptors as et_adagrad_desc (the shared front validates, sizes and packs those), and
// the checks of the weights themselves.
inline int validate_weighted_adagrad(const et_weighted_adagrad_desc* descs, int ntables,
                                     int wsize, et_adagrad_desc* ad) {
    if (ntables < 0) return fail(ET_ERR_ARG, "negative ntables");
    if (ntables > ET_MAX_TABLES_PER_LAUNCH)
        return fail(ET_ERR_ARG, "at most %d tables per update call", ET_MAX_TABLES_PER_LAUNCH);
    if (ntables > 0 && !descs) return fail(ET_ERR_ARG, "descs is NULL");
    for (int t = 0; t < ntables; ++t) {
        const et_weighted_adagrad_desc& d = descs[t];
        ad[t] = et_adagrad_desc{d.table, d.ld_table, d.nrows,         d.dim,    d.pool,
                                d.delta, d.ld_delta, d.idx,           d.ld_idx, d.batch,
                                d.cols_per_page,     d.colptr, d.nnz, d.state,  d.ld_state};
        if (!d.weights) continue;
        if (!d.colptr)
            return fail(ET_ERR_ARG, "table %d: weights need the ragged form (colptr is NULL)", t);
        if (reinterpret_cast<uintptr_t>(d.weights) % (uintptr_t)wsize != 0)
            return fail(ET_ERR_ARG, "table %d: weights not aligned to their element type", t);
    }
    return ET_OK;
}

}  // namespace et

extern "C" int et_weighted_adagrad_workspace_size(const et_weighted_adagrad_desc* descs,
                                                  int32_t ntables, int64_t* bytes) {
    et::clear_err();
    if (!bytes) return et::fail(ET_ERR_ARG, "bytes is NULL");
    et_adagrad_desc ad[ET_MAX_TABLES_PER_LAUNCH];
    int rc = et::validate_weighted_adagrad(descs, ntables, 1, ad);  // sizes only
    if (rc != ET_OK) return rc;
    int64_t n;
    int pdim;
    rc = et::validate_adagrad(ET_F32, ad, ntables, true, &n, &pdim, false);
    if (rc != ET_OK) return rc;
    *bytes = et::carve_adagrad_ws(nullptr, n, pdim).bytes;  // the weights are read in place
    return ET_OK;
}

extern "C" int et_weighted_adagrad(int dtype, const et_weighted_adagrad_desc* descs,
                                   int32_t ntables, double eta, double eps, uint32_t flags,
                                   void* workspace, int64_t ws_bytes, void* stream) {
    et::clear_err();
    int rc = et::check_adagrad_call(dtype, flags);
    if (rc != ET_OK) return rc;
    et_adagrad_desc ad[ET_MAX_TABLES_PER_LAUNCH];
    rc = et::validate_weighted_adagrad(descs, ntables, dtype == ET_F64 ? 8 : 4, ad);
    if (rc != ET_OK) return rc;
    et::AdaRun run;
    rc = et::prepare_adagrad(dtype, ad, ntables, (flags & ET_FLAG_ADAGRAD_ROWWISE) != 0,
                             workspace, ws_bytes, stream, run);
    if (rc != ET_OK || run.n == 0) return rc;
    et::UpdatePack wpack = run.pack;
    bool weighted = false;
    for (int t = 0; t < ntables; ++t) {
        const void* w = et::ada_work(ad[t]) ? descs[t].weights : nullptr;
        wpack.d[t].idx = static_cast<const int64_t*>(w);
        weighted = weighted || w != nullptr;
    }
    return et::dispatch_adagrad(dtype, flags, [&](auto e, auto row, auto nt) {
        using T = typename decltype(e)::type;
        using C = typename decltype(e)::acc;
        constexpr bool ROW = decltype(row)::value, NT = decltype(nt)::value;
        if (!weighted)  // no table carries weights: et_sparse_adagrad's own launches
            return et::launch_adagrad<T, C, ROW, NT>(run, (C)eta, (C)eps);
        return et::launch_weighted_adagrad<T, C, ROW, NT>(run, wpack, (C)eta, (C)eps);
    });
}
