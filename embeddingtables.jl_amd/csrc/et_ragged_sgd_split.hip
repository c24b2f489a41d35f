// et_ragged_sgd_split.hip — split sparse SGD over ragged and weighted gradients
// (et_ragged_sgd_split), textually included by et_update.hip after et_weighted_adagrad.hip.
// The opt-in counterpart of et_ragged_sgd / et_weighted_sgd for skewed data: a hot column is
// ordered partial sums of kChunk entries spread over the grid, not one serial chain on one wave.
//
// Semantics (include/embtab.h): the gradient sum g of et_weighted_adagrad (per chunk p_c = +0,
// t = C(w_k) * C(delta[:, bag(k)]), p_c = p_c + t for the covered entries in order;
// g = ((p_0 + p_1) + p_2) + ... in chunk order), then the update of sgd_apply_t.  An entry no
// bag covers adds nothing, keeps its list position, and its weight is never read; a column
// with no participating entry is not written.
//
// The front of the pipeline is prepare_adagrad's without an optimiser state (prepare_split:
// k_ragged_bag_ids, then group_occurrences with chunk = kChunk over the values as a vector
// index), and the workspace is carve_adagrad_ws of the same sizes.  The gradient sums reuse
// ada_occ_wsum (a NULL weight pointer counts every entry 1: x * 1 is x, so a table without
// weights gets the sums of the unweighted rule bit for bit).  The chunk and combine kernels
// below are new: they carry no state rows and end in the SGD apply step.  As in
// et_weighted_adagrad the weights ride in d[t].idx of a copied pack, read only for covered
// entries.

namespace et {

// The update of one column from its gradient sum g; x is the table column, loaded by the
// caller.
template <int D, int MODE, bool NT>
__device__ __forceinline__ void split_apply_row(
    float* __restrict__ w, const u32x4 (&x)[(D / 4 < 64 ? 1 : D / 4 / 64)],
    const float (&g)[(D / 4 < 64 ? 1 : D / 4 / 64)][4], int sub, int vpr, float eta32,
    double eta64) {
    constexpr int VPR = D / 4;
    constexpr int LPR = VPR < 64 ? VPR : 64;
    constexpr int NV = VPR / LPR;
    u32x4* wp = reinterpret_cast<u32x4*>(w) + sub;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        u32x4 y;
        y.x = __float_as_uint(
            sgd_apply_t<float, float, MODE>(__uint_as_float(x[v].x), g[v][0], eta32, eta64));
        y.y = __float_as_uint(
            sgd_apply_t<float, float, MODE>(__uint_as_float(x[v].y), g[v][1], eta32, eta64));
        y.z = __float_as_uint(
            sgd_apply_t<float, float, MODE>(__uint_as_float(x[v].z), g[v][2], eta32, eta64));
        y.w = __float_as_uint(
            sgd_apply_t<float, float, MODE>(__uint_as_float(x[v].w), g[v][3], eta32, eta64));
        if (sub + v * LPR < vpr) store16<NT>(wp + v * LPR, y);
    }
}

// Chunk pass (Float32 rows of 16-byte multiples, capacity D): lane group q of the grid takes
// chunk records q, q + groups, ...  pack.d[t].idx holds table t's weights (NULL: none).
template <int D, int MODE, bool NT>
__global__ __launch_bounds__(256) void k_ragged_sgd_chunks(
    UpdatePack pack, int ntables, const uint32_t* __restrict__ vals,
    const ChunkRec* __restrict__ recs, const uint32_t* __restrict__ counters,
    const uint32_t* __restrict__ bag_ids, float* __restrict__ partials,
    uint32_t* __restrict__ pany, int pdim, uint32_t sent, float eta32, double eta64,
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
        const int vpr = d.dim / 4;
        int vix[NV];
        vec_index<LPR, NV>(sub, vpr, vix);
        const bool apply = r.dst == kApply;
        u32x4 x[NV];
#pragma unroll
        for (int v = 0; v < NV; ++v) x[v] = u32x4{0u, 0u, 0u, 0u};
        if (apply) {  // the column first: its latency hides under the gathers
#pragma unroll
            for (int v = 0; v < NV; ++v) x[v] = reinterpret_cast<const u32x4*>(w)[vix[v]];
        }
        float acc[NV][4];
#pragma unroll
        for (int v = 0; v < NV; ++v) acc[v][0] = acc[v][1] = acc[v][2] = acc[v][3] = 0.0f;
        const bool any = ada_occ_wsum<D, U>(
            reinterpret_cast<const float*>(d.delta), (uint64_t)d.ld_delta, pack.occ_off[t], 1u,
            true, ada_weights<float>(d), bag_ids, vals, r.s0, r.s1, g, sub, vpr, acc);
        if (apply) {
            if (any)  // no participating entry: the column is not written
                split_apply_row<D, MODE, NT>(w, x, acc, sub, vpr, eta32, eta64);
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

// Combine pass: lane group q takes the multi-chunk columns q, q + groups, ... of the list,
// loads the column, adds its partial rows serially in chunk order (sixteen 16-byte loads per
// lane in flight) and applies.
template <int D, int MODE, bool NT>
__global__ __launch_bounds__(256) void k_ragged_sgd_combine(
    UpdatePack pack, int ntables, const uint32_t* __restrict__ keys,
    const uint32_t* __restrict__ seg_start, const uint32_t* __restrict__ partial_start,
    const uint32_t* __restrict__ counters, const uint32_t* __restrict__ mlist,
    const float* __restrict__ partials, const uint32_t* __restrict__ pany, int pdim, uint32_t sent,
    float eta32, double eta64, uint32_t my_mask) {
    constexpr int VPR = D / 4;
    constexpr int LPR = VPR < 64 ? VPR : 64;
    constexpr int NV = VPR / LPR;
    constexpr int GPW = 64 / LPR;
    constexpr int U = NV >= 16 ? 1 : 16 / NV;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = lane / LPR, sub = lane % LPR;
    const uint32_t M = counters[kCntM];
    const uint32_t ngroups = gridDim.x * 4u * GPW;
    for (uint32_t m = (blockIdx.x * 4u + wave) * GPW + g; m < M; m += ngroups) {
        const uint32_t seg = mlist[m];
        const uint32_t key = keys[seg_start[seg]];
        if (key >= sent) continue;
        const int t = table_of_key(pack, ntables, key);
        if (!((my_mask >> t) & 1u)) continue;
        const et_update_desc& d = pack.d[t];
        const uint32_t row = key - pack.row_off[t];
        float* w = col_ptr<float>(d.table, d.ld_table, d.cols_per_page, row);
        const int vpr = d.dim / 4;
        int vix[NV];
        vec_index<LPR, NV>(sub, vpr, vix);
        u32x4 x[NV];
#pragma unroll
        for (int v = 0; v < NV; ++v) x[v] = reinterpret_cast<const u32x4*>(w)[vix[v]];
        const uint32_t p0 = partial_start[seg], np = partial_start[seg + 1] - p0;
        float acc[NV][4];
        uint32_t any = pany[p0];
        {
            const u32x4* pp = reinterpret_cast<const u32x4*>(partials + (uint64_t)p0 * pdim);
#pragma unroll
            for (int v = 0; v < NV; ++v) {
                const u32x4 b = pp[vix[v]];
                acc[v][0] = __uint_as_float(b.x), acc[v][1] = __uint_as_float(b.y);
                acc[v][2] = __uint_as_float(b.z), acc[v][3] = __uint_as_float(b.w);
            }
        }
        for (uint32_t q0 = 1; q0 < np; q0 += U) {
            u32x4 buf[U][NV];
            uint32_t a[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const uint32_t q = p0 + (q0 + u < np ? q0 + u : np - 1);
                const u32x4* pp = reinterpret_cast<const u32x4*>(partials + (uint64_t)q * pdim);
                a[u] = pany[q];
#pragma unroll
                for (int v = 0; v < NV; ++v) buf[u][v] = pp[vix[v]];
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (q0 + u >= np) continue;
                any |= a[u];
#pragma unroll
                for (int v = 0; v < NV; ++v) {
                    acc[v][0] = acc[v][0] + __uint_as_float(buf[u][v].x);
                    acc[v][1] = acc[v][1] + __uint_as_float(buf[u][v].y);
                    acc[v][2] = acc[v][2] + __uint_as_float(buf[u][v].z);
                    acc[v][3] = acc[v][3] + __uint_as_float(buf[u][v].w);
                }
            }
        }
        if (any) split_apply_row<D, MODE, NT>(w, x, acc, sub, vpr, eta32, eta64);
    }
}

// Generic path: one wave per chunk record or multi-chunk column, lane l holds features
// f0 + l + 64 k, k < kAdaK (et_adagrad.hip).  sum_block(f0, acc) fills the block's gradient
// sums and returns whether any entry took part (wave-uniform).
template <typename T, typename C, int MODE, bool NT, typename F>
__device__ __forceinline__ void split_apply_generic(T* __restrict__ w, int dim, int lane, C eta_c,
                                                    double eta64, F&& sum_block) {
    C acc[kAdaK];
    for (int f0 = 0; f0 < dim; f0 += 64 * kAdaK) {
        if (!sum_block(f0, acc)) return;  // no participating entry: the column is not written
#pragma unroll
        for (int k = 0; k < kAdaK; ++k) {
            const int f = f0 + lane + 64 * k;
            if (f < dim)
                store_scalar<NT>(w + f, sgd_apply_t<T, C, MODE>(w[f], acc[k], eta_c, eta64));
        }
    }
}

template <typename T, typename C, int MODE, bool NT>
__global__ __launch_bounds__(256) void k_ragged_sgd_chunks_generic(
    UpdatePack pack, int ntables, const uint32_t* __restrict__ vals,
    const ChunkRec* __restrict__ recs, const uint32_t* __restrict__ counters,
    const uint32_t* __restrict__ bag_ids, C* __restrict__ partials, uint32_t* __restrict__ pany,
    int pdim, uint32_t sent, C eta_c, double eta64) {
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
        const uint32_t occ_off = pack.occ_off[t];
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
                    myb = bag_ids[o];
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
                        if (b[j] == 0u) continue;  // past the chunk, or an entry no bag covers
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
        T* w = col_ptr<T>(d.table, d.ld_table, d.cols_per_page,
                          (uint64_t)(r.key - pack.row_off[t]));
        split_apply_generic<T, C, MODE, NT>(w, dim, lane, eta_c, eta64, sum_block);
    }
}

template <typename T, typename C, int MODE, bool NT>
__global__ __launch_bounds__(256) void k_ragged_sgd_combine_generic(
    UpdatePack pack, int ntables, const uint32_t* __restrict__ keys,
    const uint32_t* __restrict__ seg_start, const uint32_t* __restrict__ partial_start,
    const uint32_t* __restrict__ counters, const uint32_t* __restrict__ mlist,
    const C* __restrict__ partials, const uint32_t* __restrict__ pany, int pdim, uint32_t sent,
    C eta_c, double eta64) {
    const int lane = threadIdx.x & 63;
    const uint32_t M = counters[kCntM];
    const uint32_t waves = gridDim.x * 4;
    for (uint32_t m = blockIdx.x * 4 + (threadIdx.x >> 6); m < M; m += waves) {
        const uint32_t seg = mlist[m];
        const uint32_t key = keys[seg_start[seg]];
        if (key >= sent) continue;
        const int t = table_of_key(pack, ntables, key);
        if ((pack.vec_mask >> t) & 1u) continue;
        const et_update_desc& d = pack.d[t];
        const int dim = d.dim;
        const uint32_t p0 = partial_start[seg], np = partial_start[seg + 1] - p0;
        auto sum_block = [&](int f0, C(&acc)[kAdaK]) -> bool {
            uint32_t any = pany[p0];
#pragma unroll
            for (int k = 0; k < kAdaK; ++k) {
                const int f = f0 + lane + 64 * k;
                acc[k] = f < dim ? partials[(uint64_t)p0 * pdim + f] : C(0);
            }
            for (uint32_t q0 = 1; q0 < np; q0 += kAdaE) {
                C x[kAdaE][kAdaK];
                uint32_t a[kAdaE];
#pragma unroll
                for (int j = 0; j < kAdaE; ++j) {
                    const bool in = q0 + j < np;
                    a[j] = in ? pany[p0 + q0 + j] : 0u;
#pragma unroll
                    for (int k = 0; k < kAdaK; ++k) {
                        const int f = f0 + lane + 64 * k;
                        x[j][k] = in && f < dim ? partials[(uint64_t)(p0 + q0 + j) * pdim + f] : C(0);
                    }
                }
#pragma unroll
                for (int j = 0; j < kAdaE; ++j) {
                    if (q0 + j >= np) continue;
                    any |= a[j];
#pragma unroll
                    for (int k = 0; k < kAdaK; ++k) acc[k] = acc[k] + x[j][k];
                }
            }
            return any != 0u;
        };
        T* w = col_ptr<T>(d.table, d.ld_table, d.cols_per_page, (uint64_t)(key - pack.row_off[t]));
        split_apply_generic<T, C, MODE, NT>(w, dim, lane, eta_c, eta64, sum_block);
    }
}

// Host --------------------------------------------------------------------------------------

struct SplitRun {
    UpdatePack pack;  // the values as a vector index; d[t].idx holds the weights after the front
    AdaWs w;
    Grouped gr;
    VecGroups vg;
    int ntables, pdim;
    int64_t n;
    uint32_t sent;
    bool any_generic;
    hipStream_t s;
};

inline bool split_work(const et_weighted_update_desc& d) {
    return d.nnz > 0 && d.batch > 0 && d.dim > 0;
}

// Every descriptor check of et_weighted_sgd (a table may come without weights here), the
// entries of all tables with work and the partial rows' width: the size query and the call
// both size their workspace from this.
inline int validate_split(const et_weighted_update_desc* descs, int ntables, int wsize,
                          bool need_ptrs, int64_t* n_out, int* pdim_out) {
    et_ragged_update_desc rd[ET_MAX_TABLES_PER_LAUNCH];
    int rc = validate_weighted_update(descs, ntables, rd, n_out, need_ptrs);
    if (rc != ET_OK) return rc;
    int pdim = 0;
    for (int t = 0; t < ntables; ++t) {
        const et_weighted_update_desc& d = descs[t];
        if (!split_work(d)) continue;
        if (d.dim > pdim) pdim = d.dim;
        if (need_ptrs && d.weights && reinterpret_cast<uintptr_t>(d.weights) % (uintptr_t)wsize != 0)
            return fail(ET_ERR_ARG, "table %d: weights not aligned to their element type", t);
    }
    *pdim_out = (pdim + 3) & ~3;
    return ET_OK;
}

// prepare_adagrad without an optimiser state: the workspace, the tables packed as vector
// indices over their values, the bag id of every entry and group_occurrences.
inline int prepare_split(int dtype, const et_weighted_update_desc* descs, int ntables,
                         void* workspace, int64_t ws_bytes, void* stream, SplitRun& run) {
    run.w = carve_adagrad_ws(static_cast<char*>(workspace), run.n, run.pdim);
    if (!workspace || ws_bytes < run.w.bytes)
        return fail(ET_ERR_WORKSPACE, "workspace of %lld bytes needed", (long long)run.w.bytes);
    run.ntables = ntables;
    run.s = static_cast<hipStream_t>(stream);

    UpdatePack& pack = run.pack;
    RaggedBagArgs ba{};
    uint32_t ro = 0, oo = 0;
    int64_t max_batch = 0;
    pack.vec_mask = 0;
    run.any_generic = false;
    for (int t = 0; t < ntables; ++t) {
        const et_weighted_update_desc& a = descs[t];
        const bool work = split_work(a);
        et_update_desc d{};
        d.table = a.table;
        d.ld_table = a.ld_table;
        d.nrows = a.nrows;
        d.dim = a.dim;
        d.pool = 1;
        d.delta = a.delta;
        d.ld_delta = a.ld_delta;
        d.idx = a.idx;
        d.ld_idx = 1;
        d.batch = work ? a.nnz : 0;
        d.cols_per_page = a.cols_per_page;
        pack.d[t] = d;
        pack.row_off[t] = ro;
        pack.occ_off[t] = oo;
        ba.colptr[t] = a.colptr;
        ba.batch[t] = work ? a.batch : 0;
        ba.nnz[t] = work ? a.nnz : 0;
        ba.off[t] = (int64_t)oo;
        ro += (uint32_t)a.nrows;
        oo += (uint32_t)d.batch;
        if (!work) continue;
        if (a.batch > max_batch) max_batch = a.batch;
        // the vector kernels: Float32 rows and gradient rows of 16-byte multiples
        const bool vec = dtype == ET_F32 && (a.cols_per_page > 0 || aligned16(a.table)) &&
                         a.ld_table % 4 == 0 && a.dim % 4 == 0 && a.dim <= 2048 &&
                         aligned16(a.delta) && a.ld_delta % 4 == 0;
        if (vec && run.vg.add(vec_dim_ok(a.dim) ? a.dim : masked_capacity(a.dim), t))
            pack.vec_mask |= 1u << t;
        else
            run.any_generic = true;
    }
    pack.row_off[ntables] = ro;
    pack.occ_off[ntables] = oo;
    run.sent = ro;  // key of out-of-range indices (sorts last)

    ET_HIP_CHECK(hipMemsetAsync(run.w.bag, 0, (size_t)run.n * 4, run.s));
    int rc = launch_ragged_bag_ids<uint32_t>(ba, ntables, max_batch, run.w.bag, run.s);
    if (rc != ET_OK) return rc;
    rc = group_occurrences(pack, ntables, run.n, run.sent, kChunk, run.w.u, run.gr, run.s);
    if (rc != ET_OK) return rc;
    // the key pass was the last reader of idx: from here on it holds the weights
    for (int t = 0; t < ntables; ++t)
        pack.d[t].idx =
            static_cast<const int64_t*>(split_work(descs[t]) ? descs[t].weights : nullptr);
    return ET_OK;
}

template <typename T, typename C, int MODE, bool NT>
int launch_ragged_sgd_split(const SplitRun& r, C eta_c, double eta64) {
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
                hipLaunchKernelGGL((k_ragged_sgd_chunks<D, MODE, NT>), dim3(grid), dim3(256), 0,
                                   r.s, r.pack, r.ntables, r.gr.vals, u.recs, u.counters, r.w.bag,
                                   partials, r.w.pany, r.pdim, r.sent, eta_c, eta64, r.vg.mask[i]);
                hipLaunchKernelGGL((k_ragged_sgd_combine<D, MODE, NT>),
                                   dim3((unsigned)(cb < 2048 ? cb : 2048)), dim3(256), 0, r.s,
                                   r.pack, r.ntables, r.gr.keys, u.seg_start, u.multi, u.counters,
                                   u.mlist, partials, r.w.pany, r.pdim, r.sent, eta_c, eta64,
                                   r.vg.mask[i]);
            });
        ET_LAUNCH_CHECK("k_ragged_sgd_chunks");
    }
    if (r.any_generic) {
        C* partials = reinterpret_cast<C*>(r.w.partials);
        const int64_t cb = cdiv64(mmax, 4);
        hipLaunchKernelGGL((k_ragged_sgd_chunks_generic<T, C, MODE, NT>), dim3(grid), dim3(256), 0,
                           r.s, r.pack, r.ntables, r.gr.vals, u.recs, u.counters, r.w.bag,
                           partials, r.w.pany, r.pdim, r.sent, eta_c, eta64);
        hipLaunchKernelGGL((k_ragged_sgd_combine_generic<T, C, MODE, NT>),
                           dim3((unsigned)(cb < 4096 ? cb : 4096)), dim3(256), 0, r.s, r.pack,
                           r.ntables, r.gr.keys, u.seg_start, u.multi, u.counters, u.mlist,
                           partials, r.w.pany, r.pdim, r.sent, eta_c, eta64);
        ET_LAUNCH_CHECK("k_ragged_sgd_chunks_generic");
    }
    return ET_OK;
}

}  // namespace et

extern "C" int et_ragged_sgd_split_workspace_size(const et_weighted_update_desc* descs,
                                                  int32_t ntables, int64_t* bytes) {
    et::clear_err();
    if (!bytes) return et::fail(ET_ERR_ARG, "bytes is NULL");
    int64_t n;
    int pdim;
    const int rc = et::validate_split(descs, ntables, 1, false, &n, &pdim);  // sizes only
    if (rc != ET_OK) return rc;
    *bytes = et::carve_adagrad_ws(nullptr, n, pdim).bytes;  // the weights are read in place
    return ET_OK;
}

extern "C" int et_ragged_sgd_split(int dtype, const et_weighted_update_desc* descs,
                                   int32_t ntables, double eta, uint32_t flags, void* workspace,
                                   int64_t ws_bytes, void* stream) {
    et::clear_err();
    if (dtype != ET_F32 && dtype != ET_F64 && dtype != ET_F16 && dtype != ET_BF16)
        return et::fail(ET_ERR_UNSUPPORTED, "split ragged SGD: dtype %d", dtype);
    if (flags & ET_FLAG_EXACT_UPDATE)
        return et::fail(ET_ERR_ARG, "split ragged SGD is never exact: use et_ragged_sgd or "
                                    "et_weighted_sgd for the serial sum");
    if (flags & (ET_FLAG_SGD_INDEX_ONLY | ET_FLAG_SGD_APPLY_ONLY | ET_FLAG_SGD_HOT_PASS |
                 ET_FLAG_ADAGRAD_ROWWISE))
        return et::fail(ET_ERR_UNSUPPORTED, "split ragged SGD has no phased form, no hot-column "
                                            "pass and no row-wise form");
    et::SplitRun run;
    int rc = et::validate_split(descs, ntables, dtype == ET_F64 ? 8 : 4, true, &run.n, &run.pdim);
    if (rc != ET_OK || run.n == 0) return rc;
    rc = et::prepare_split(dtype, descs, ntables, workspace, ws_bytes, stream, run);
    if (rc != ET_OK) return rc;

    // Float16 sums in Float32: ET_FLAG_F16_FP32_ACC is implied
    const double eta_c = et::convert_eta(dtype, eta);
    return et::dispatch_sgd(dtype, flags | ET_FLAG_F16_FP32_ACC, [&](auto e, auto mode, auto nt) {
        using T = typename decltype(e)::type;
        using C = typename decltype(e)::acc;
        if constexpr (sizeof(C) == 2) {  // never selected: the flag above picks Float32 sums
            return et::fail(ET_ERR_UNSUPPORTED, "split ragged SGD sums Float16 in Float32");
        } else {
            return et::launch_ragged_sgd_split<T, C, decltype(mode)::value, decltype(nt)::value>(
                run, (C)eta_c, eta);
        }
    });
}
