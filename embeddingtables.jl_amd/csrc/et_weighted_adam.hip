// et_weighted_adam.hip — sparse Adam over gradients that carry a weight per entry
// (et_weighted_adam), textually included by et_update.hip after et_adam.hip.  The front of the
// pipeline (pack_adagrad_tables with Adam's AdaFrontOpts), k_adam_advance, the combine kernels
// and the apply step are et_sparse_adam's, unchanged; the chunk pass is new, and so is the way
// it learns what to gather.
//
// Semantics (include/embtab.h): the gradient sum g of a table that carries weights is
// et_weighted_adagrad's rule (per chunk p_c = +0, then t = C(w_k) * C(delta[:, bag(k)]),
// p_c = p_c + t for every covered entry in order, two roundings, never an fma; the chunks added
// in chunk order); everything behind g is et_sparse_adam's.
//
// Why not et_weighted_adagrad's move.  Its chunk kernels take the weights in the idx slot of
// their UpdatePack copy.  The Adam kernels already keep m / ld_m there, and their argument
// block (UpdatePack 3,088 + AdamPack 776 bytes and the scalars) has no room for 32 more
// pointers under the 4 KiB of a launch.  So the weights reach the chunk pass as data:
//
//   k_wadam_pairs<C>   one pass over the sorted occurrence list, after group_occurrences.  List
//                      position i holds occurrence o = vals[i]; the kernel finds o's table from
//                      occ_off, resolves the bag (ada_bag) and reads the weight w[o - occ_off[t]]
//                      only when a bag covers the entry and the table has weights (otherwise
//                      1.0), and writes pairs[i] = (bag, weight).  It takes the UpdatePack copy
//                      with the weights in idx and needs no m: its arguments fit.
//                      C = Float32: one 8-byte word (bag, bits(weight)).  C = Float64: one
//                      16-byte record (bag, 0, weight) -- one record, not two arrays, so the
//                      chunk pass fetches an entry with a single load.
//   k_wadam_chunks<D>  Float32 tables under k_adam_chunks' conditions, in its lane-group layout
//                      and capacities.  A chunk record's [s0, s1) is a contiguous run of pairs:
//                      each lane loads one pair per round with one coalesced 8-byte load (the
//                      unweighted kernel's vals[i] -> bag_ids[o] is a dependent pair of loads,
//                      and a weight would be a third), writes it to its group's slot table in
//                      LDS with one 64-bit write, and every gathered row then costs the group one
//                      broadcast 64-bit LDS read at an immediate offset -- against two cross-lane
//                      shuffles per row in ada_occ_wsum.  A wave's LDS operations retire in
//                      order, so there is no __syncthreads, only a compiler fence
//                      (wadam_wave_fence).  w, m, v and the step are loaded before the gather,
//                      eight 16-byte gradient loads per lane stay in flight.  The kernel takes
//                      neither vals, bag_ids nor a weights pointer.
//   k_wadam_chunks_generic  every other element type, dim and alignment: one wave per record,
//                      lanes over features, the same pair stream (one coalesced load of 64
//                      pairs, handed out by lane shuffles).
//
// Slot tables: each wave owns GPW tables of LPR pairs, LPR + 1 pairs apart: an odd number of
// 8-byte words, so the GPW addresses of one broadcast read fall on different banks (with a
// stride of LPR pairs groups g and g + 32 / (2 LPR) would share banks at different addresses).
//
// Workspace: et_adam_workspace_size of the same sizes, then the pair stream, 16 bytes per
// occurrence whatever C is (the size function is not told the element type), rounded up to 256.

namespace et {

template <typename C>
struct WPair;
template <>
struct alignas(8) WPair<float> {
    uint32_t bag;  // 1-based gradient column, 0: no bag covers the entry
    float w;
};
template <>
struct alignas(16) WPair<double> {
    uint32_t bag;
    uint32_t zero;
    double w;
};
constexpr int64_t kWPairBytes = 16;  // workspace bytes per occurrence, either C

inline int64_t wadam_pairs_bytes(int64_t n) { return align256(kWPairBytes * n); }

template <typename C>
__global__ __launch_bounds__(256) void k_wadam_pairs(UpdatePack wpack, int ntables,
                                                     uint32_t ragged,
                                                     const uint32_t* __restrict__ vals,
                                                     const uint32_t* __restrict__ bag_ids,
                                                     WPair<C>* __restrict__ pairs, uint32_t n) {
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
        const uint32_t o = vals[i];
        int t = 0;  // tables without work have an empty occurrence range and are stepped over
        while (t + 1 < ntables && o >= wpack.occ_off[t + 1]) ++t;
        const et_update_desc& d = wpack.d[t];
        const uint32_t off = wpack.occ_off[t];
        const C* __restrict__ wt = ada_weights<C>(d);
        WPair<C> p{};
        p.bag = ada_bag(o, (ragged >> t) & 1u, off, (uint32_t)d.pool, bag_ids);
        p.w = wt != nullptr && p.bag != 0u ? wt[o - off] : C(1);
        pairs[i] = p;
    }
}

// Compiler-only ordering of one wave's LDS writes and reads, as qw_wave_fence in
// et_quant_weighted.hip (no instruction: a wave's LDS operations retire in issue order).
__device__ __forceinline__ void wadam_wave_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// acc += w_k * delta[:, bag(k)] over the pairs [s0, s1) in order (one lane group).  Per round
// the group loads LPR pairs, one per lane, and parks them in `slots` (its slot table); a lane
// past the end parks bag 0.  U gradient rows are loaded before the first multiply.  Control
// flow is uniform inside a lane group, not inside a wave.  Returns whether any entry took part.
template <int D, int U>
__device__ __forceinline__ bool wadam_pair_sum(const float* __restrict__ delta, uint64_t ldd,
                                               const uint2* __restrict__ pairs, uint2* slots,
                                               uint32_t s0, uint32_t s1, int sub, int vpr,
                                               float (&acc)[(D / 4 < 64 ? 1 : D / 4 / 64)][4]) {
    constexpr int VPR = D / 4;
    constexpr int LPR = VPR < 64 ? VPR : 64;
    constexpr int NV = VPR / LPR;
    int vix[NV];
    vec_index<LPR, NV>(sub, vpr, vix);
    bool any = false;
    for (uint32_t c0 = s0; c0 < s1; c0 += LPR) {
        const int cnt = (int)(s1 - c0 < (uint32_t)LPR ? s1 - c0 : (uint32_t)LPR);
        uint2 mine = make_uint2(0u, 0u);
        if (sub < cnt) mine = pairs[c0 + (uint32_t)sub];
        slots[sub] = mine;
        wadam_wave_fence();
        for (int i0 = 0; i0 < cnt; i0 += U) {
            uint32_t b[U];
            float wk[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if constexpr (LPR >= U) {  // i0 is a multiple of U and LPR one of U: a slot
                    const uint2 pr = slots[i0 + u];
                    b[u] = pr.x;
                    wk[u] = __uint_as_float(pr.y);
                } else {
                    const int j = i0 + u;
                    const uint2 pr = slots[j < LPR ? j : LPR - 1];
                    b[u] = j < LPR ? pr.x : 0u;
                    wk[u] = __uint_as_float(pr.y);
                }
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
        wadam_wave_fence();  // the next round's writes stay behind these reads
    }
    return any;
}

// Chunk pass over the pair stream: lane group q of the grid takes chunk records q, q + groups,
// ...  `pack` is the UpdatePack copy with m / ld_m in idx / ld_idx, as in k_adam_chunks.
template <int D, bool ROW, bool NT>
__global__ ET_ADAM_KERNEL __launch_bounds__(256) void k_wadam_chunks(
    UpdatePack pack, AdamPack ap, int ntables, const uint2* __restrict__ pairs,
    const ChunkRec* __restrict__ recs, const uint32_t* __restrict__ counters,
    float* __restrict__ partials, uint32_t* __restrict__ pany, int pdim, uint32_t sent,
    AdamHyper<float> h, uint32_t my_mask) {
    constexpr int VPR = D / 4;
    constexpr int LPR = VPR < 64 ? VPR : 64;
    constexpr int NV = VPR / LPR;
    constexpr int GPW = 64 / LPR;
    constexpr int U = NV >= 8 ? 1 : 8 / NV;
    constexpr int STRIDE = LPR + 1;
    __shared__ uint2 s_slots[4 * GPW * STRIDE];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = lane / LPR, sub = lane % LPR;
    uint2* slots = s_slots + (wave * GPW + g) * STRIDE;  // this group's slot table
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
        float* mp = adam_m_ptr<float>(d, row);
        float* vp = reinterpret_cast<float*>(ap.v[t]) +
                    (ROW ? (uint64_t)row : (uint64_t)row * (uint64_t)ap.ld_v[t]);
        const int vpr = d.dim / 4;
        int vix[NV];
        vec_index<LPR, NV>(sub, vpr, vix);
        const bool apply = r.dst == kApply;
        u32x4 x[NV], mo[NV], vo[NV];
        float vrow = 0.0f, c1 = 1.0f, c2 = 1.0f;
#pragma unroll
        for (int v = 0; v < NV; ++v) x[v] = mo[v] = vo[v] = u32x4{0u, 0u, 0u, 0u};
        if (apply) {  // three row streams first: their latency hides under the gathers
#pragma unroll
            for (int v = 0; v < NV; ++v) x[v] = reinterpret_cast<const u32x4*>(w)[vix[v]];
#pragma unroll
            for (int v = 0; v < NV; ++v) mo[v] = reinterpret_cast<const u32x4*>(mp)[vix[v]];
            if constexpr (ROW) {
                vrow = *vp;
            } else {
#pragma unroll
                for (int v = 0; v < NV; ++v) vo[v] = reinterpret_cast<const u32x4*>(vp)[vix[v]];
            }
            const float* st = reinterpret_cast<const float*>(ap.step[t]);
            c1 = 1.0f - st[0];
            c2 = 1.0f - st[1];
        }
        float acc[NV][4];
#pragma unroll
        for (int v = 0; v < NV; ++v) acc[v][0] = acc[v][1] = acc[v][2] = acc[v][3] = 0.0f;
        const bool any = wadam_pair_sum<D, U>(reinterpret_cast<const float*>(d.delta),
                                              (uint64_t)d.ld_delta, pairs, slots, r.s0, r.s1, sub,
                                              vpr, acc);
        if (apply) {
            if (any)  // no participating entry: neither the column nor its moments are written
                adam_apply_row<D, ROW, NT>(w, mp, vp, x, mo, vo, vrow, acc, sub, vpr, d.dim, c1, c2,
                                           h);
        } else {
            u32x4* pp = reinterpret_cast<u32x4*>(partials + (uint64_t)r.dst * pdim) + sub;
#pragma unroll
            for (int v = 0; v < NV; ++v)
                if (sub + v * LPR < vpr) pp[v * LPR] = adam_pack(acc[v]);
            if (sub == 0) pany[r.dst] = any ? 1u : 0u;
        }
    }
}

// Generic path: the weighted gradient sums of features f0 + lane + 64 k over the pairs
// [s0, s1), kAdaE gradient rows in flight (adam_occ_block over the pair stream).
template <typename T, typename C>
__device__ __forceinline__ bool wadam_pair_block(const T* __restrict__ delta, uint64_t ldd,
                                                 int dim, const WPair<C>* __restrict__ pairs,
                                                 uint32_t s0, uint32_t s1, int lane, int f0,
                                                 C (&acc)[kAdaK]) {
#pragma unroll
    for (int k = 0; k < kAdaK; ++k) acc[k] = C(0);
    bool any = false;
    for (uint32_t e0 = s0; e0 < s1; e0 += 64) {
        const uint32_t cnt = s1 - e0 < 64u ? s1 - e0 : 64u;
        uint32_t myb = 0;
        C myw = C(1);
        if ((uint32_t)lane < cnt) {
            const WPair<C> p = pairs[e0 + (uint32_t)lane];
            myb = p.bag;
            myw = p.w;
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
                    x[j][k] = b[j] != 0u && f < dim ? delta[(uint64_t)(b[j] - 1u) * ldd + f] : T(0);
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
}

template <typename T, typename C, bool ROW, bool NT>
__global__ ET_ADAM_KERNEL __launch_bounds__(256) void k_wadam_chunks_generic(
    UpdatePack pack, AdamPack ap, int ntables, const WPair<C>* __restrict__ pairs,
    const ChunkRec* __restrict__ recs, const uint32_t* __restrict__ counters,
    C* __restrict__ partials, uint32_t* __restrict__ pany, int pdim, uint32_t sent,
    AdamHyper<C> h) {
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
        const uint64_t ldd = (uint64_t)d.ld_delta;
        const uint32_t s0 = r.s0, s1 = r.s1;
        auto sum_block = [&](int f0, C(&acc)[kAdaK]) __attribute__((always_inline)) -> bool {
            return wadam_pair_block<T, C>(delta, ldd, dim, pairs, s0, s1, lane, f0, acc);
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
        C* vp = reinterpret_cast<C*>(ap.v[t]) +
                (ROW ? (uint64_t)row : (uint64_t)row * (uint64_t)ap.ld_v[t]);
        const C* st = reinterpret_cast<const C*>(ap.step[t]);
        adam_apply_generic<T, C, ROW, NT>(w, adam_m_ptr<C>(d, row), vp, dim, lane, C(1) - st[0],
                                          C(1) - st[1], h, sum_block);
    }
}

// Host --------------------------------------------------------------------------------------

// launch_adam with the pair pass in front and the pair-stream chunk kernels; `mpack` carries
// m in idx (the chunk and combine kernels), `wpack` the weights (the pair pass only).  The
// combine kernels are et_sparse_adam's: the partial rows are already weighted.
template <typename T, typename C, bool ROW, bool NT>
int launch_weighted_adam(const AdaRun& r, const UpdatePack& mpack, const UpdatePack& wpack,
                         const AdamPack& ap, AdamHyper<C> h, void* pair_ws) {
    hipLaunchKernelGGL((k_adam_advance<C>), dim3(1), dim3(64), 0, r.s, ap, r.ntables, h.b1, h.b2);
    ET_LAUNCH_CHECK("k_adam_advance");
    WPair<C>* pairs = static_cast<WPair<C>*>(pair_ws);
    const int64_t pb = cdiv64(r.n, 1024);  // four list positions a thread
    hipLaunchKernelGGL((k_wadam_pairs<C>), dim3((unsigned)(pb < 16384 ? pb : 16384)), dim3(256), 0,
                       r.s, wpack, r.ntables, ap.ragged, r.gr.vals, r.w.bag, pairs,
                       (uint32_t)r.n);
    ET_LAUNCH_CHECK("k_wadam_pairs");
    const unsigned grid = sgd_grid(r.n);
    const int64_t mmax = r.n / kChunk + 2;  // multi-chunk columns at most
    const UpdateWs& u = r.w.u;
    if constexpr (__is_same(T, float)) {
        float* partials = reinterpret_cast<float*>(r.w.partials);
        for (int i = 0; i < r.vg.n; ++i)
            with_adam_capacity(r.vg.cap[i], [&](auto cap) {
                constexpr int D = decltype(cap)::value;
                constexpr int GPW = D / 4 < 64 ? 64 / (D / 4) : 1;
                const int64_t cb = cdiv64(mmax, 4 * GPW);
                hipLaunchKernelGGL((k_wadam_chunks<D, ROW, NT>), dim3(grid), dim3(256), 0, r.s,
                                   mpack, ap, r.ntables, reinterpret_cast<const uint2*>(pairs),
                                   u.recs, u.counters, partials, r.w.pany, r.pdim, r.sent, h,
                                   r.vg.mask[i]);
                hipLaunchKernelGGL((k_adam_combine<D, ROW, NT>),
                                   dim3((unsigned)(cb < 2048 ? cb : 2048)), dim3(256), 0, r.s,
                                   mpack, ap, r.ntables, r.gr.keys, u.seg_start, u.multi,
                                   u.counters, u.mlist, partials, r.w.pany, r.pdim, r.sent, h,
                                   r.vg.mask[i]);
            });
        ET_LAUNCH_CHECK("k_wadam_chunks");
    }
    if (r.any_generic) {
        C* partials = reinterpret_cast<C*>(r.w.partials);
        const int64_t cb = cdiv64(mmax, 4);
        hipLaunchKernelGGL((k_wadam_chunks_generic<T, C, ROW, NT>), dim3(grid), dim3(256), 0, r.s,
                           mpack, ap, r.ntables, pairs, u.recs, u.counters, partials, r.w.pany,
                           r.pdim, r.sent, h);
        hipLaunchKernelGGL((k_adam_combine_generic<T, C, ROW, NT>),
                           dim3((unsigned)(cb < 4096 ? cb : 4096)), dim3(256), 0, r.s, mpack, ap,
                           r.ntables, r.gr.keys, u.seg_start, u.multi, u.counters, u.mlist,
                           partials, r.w.pany, r.pdim, r.sent, h);
        ET_LAUNCH_CHECK("k_wadam_chunks_generic");
    }
    return ET_OK;
}

// The descriptors as et_adam_desc (the checks and the front of et_sparse_adam take those), and
// the checks of the weights themselves; wsize 1: sizes only.
inline int validate_weighted_adam(const et_weighted_adam_desc* descs, int ntables, int wsize,
                                  et_adam_desc* ad) {
    int rc = adam_table_count(reinterpret_cast<const et_adam_desc*>(descs), ntables);
    if (rc != ET_OK) return rc;
    for (int t = 0; t < ntables; ++t) {
        const et_weighted_adam_desc& d = descs[t];
        ad[t] = et_adam_desc{d.table, d.ld_table, d.nrows,         d.dim,    d.pool, d.delta,
                             d.ld_delta,          d.idx,           d.ld_idx, d.batch,
                             d.cols_per_page,     d.colptr, d.nnz, d.m,      d.ld_m, d.v,
                             d.ld_v,              d.step};
        if (!d.weights) continue;
        if (!d.colptr)
            return fail(ET_ERR_ARG, "table %d: weights need the ragged form (colptr is NULL)", t);
        if (reinterpret_cast<uintptr_t>(d.weights) % (uintptr_t)wsize != 0)
            return fail(ET_ERR_ARG, "table %d: weights not aligned to their element type", t);
    }
    return ET_OK;
}

// validate_adam_blocks knows no weights: the weights of every table with work against every
// block this call writes (tables, moments, steps), the same block sizes.
inline int validate_wadam_weight_blocks(int dtype, const et_weighted_adam_desc* descs,
                                        const et_adam_desc* ad, int ntables, bool rowwise) {
    const uint64_t es = (uint64_t)elsize(dtype), cs = dtype == ET_F64 ? 8u : 4u;
    for (int i = 0; i < ntables; ++i) {
        if (!descs[i].weights || !ada_work(adam_as_adagrad(ad[i]))) continue;
        const uintptr_t wa = (uintptr_t)descs[i].weights;
        const uint64_t wn = (uint64_t)ad[i].nnz * cs;
        for (int t = 0; t < ntables; ++t) {
            const et_adam_desc& d = ad[t];
            if (!ada_work(adam_as_adagrad(d))) continue;
            const char* hit = nullptr;
            if (ranges_overlap(wa, wn, (uintptr_t)d.step, 2 * cs)) hit = "step";
            if (d.nrows > 0) {
                const uint64_t rows1 = (uint64_t)(d.nrows - 1), dim = (uint64_t)d.dim;
                const uint64_t tbytes =
                    d.cols_per_page > 0
                        ? (uint64_t)((d.nrows + d.cols_per_page - 1) / d.cols_per_page) * 8u
                        : (rows1 * (uint64_t)d.ld_table + dim) * es;
                const uint64_t vbytes = rowwise ? (uint64_t)d.nrows * cs
                                                : (rows1 * (uint64_t)d.ld_v + dim) * cs;
                if (ranges_overlap(wa, wn, (uintptr_t)d.table, tbytes)) hit = "the table";
                if (ranges_overlap(wa, wn, (uintptr_t)d.m, (rows1 * (uint64_t)d.ld_m + dim) * cs))
                    hit = "m";
                if (ranges_overlap(wa, wn, (uintptr_t)d.v, vbytes)) hit = "v";
            }
            if (hit)
                return fail(ET_ERR_ARG, "weights of table %d overlap %s of table %d", i, hit, t);
        }
    }
    return ET_OK;
}

}  // namespace et

extern "C" int et_weighted_adam_workspace_size(const et_weighted_adam_desc* descs,
                                               int32_t ntables, int64_t* bytes) {
    et::clear_err();
    if (!bytes) return et::fail(ET_ERR_ARG, "bytes is NULL");
    et_adam_desc ad[ET_MAX_TABLES_PER_LAUNCH];
    int rc = et::validate_weighted_adam(descs, ntables, 1, ad);
    if (rc != ET_OK) return rc;
    et_adagrad_desc ag[ET_MAX_TABLES_PER_LAUNCH];
    for (int t = 0; t < ntables; ++t) ag[t] = et::adam_as_adagrad(ad[t]);
    int64_t n;
    int pdim;
    rc = et::validate_adagrad(ET_F32, ag, ntables, true, &n, &pdim, false);
    if (rc != ET_OK) return rc;
    *bytes = et::carve_adagrad_ws(nullptr, n, pdim).bytes + et::wadam_pairs_bytes(n);
    return ET_OK;
}

extern "C" int et_weighted_adam(int dtype, const et_weighted_adam_desc* descs, int32_t ntables,
                                double eta, double beta1, double beta2, double eps,
                                uint32_t flags, void* workspace, int64_t ws_bytes, void* stream) {
    et::clear_err();
    int rc = et::check_adam_call(dtype, flags, beta1, beta2);
    if (rc != ET_OK) return rc;
    et_adam_desc ad[ET_MAX_TABLES_PER_LAUNCH];
    rc = et::validate_weighted_adam(descs, ntables, dtype == ET_F64 ? 8 : 4, ad);
    if (rc != ET_OK) return rc;
    const bool rowwise = (flags & ET_FLAG_ADAM_ROWWISE) != 0;
    et_adagrad_desc ag[ET_MAX_TABLES_PER_LAUNCH];
    for (int t = 0; t < ntables; ++t) ag[t] = et::adam_as_adagrad(ad[t]);
    et::AdaRun run;
    rc = et::validate_adagrad(dtype, ag, ntables, false, &run.n, &run.pdim, true, "m");
    if (rc != ET_OK) return rc;
    rc = et::validate_adam_blocks(dtype, ad, ntables, rowwise);
    if (rc != ET_OK) return rc;
    rc = et::validate_wadam_weight_blocks(dtype, descs, ad, ntables, rowwise);
    if (rc != ET_OK || run.n == 0) return rc;
    run.w = et::carve_adagrad_ws(static_cast<char*>(workspace), run.n, run.pdim);
    const int64_t need = run.w.bytes + et::wadam_pairs_bytes(run.n);
    if (!workspace || ws_bytes < need)
        return et::fail(ET_ERR_WORKSPACE, "workspace of %lld bytes needed", (long long)need);
    void* pair_ws = static_cast<char*>(workspace) + run.w.bytes;  // 256-byte aligned, as the rest
    et::AdaFrontOpts fo;
    fo.vec_max_dim = ET_ADAM_VEC_MAX_DIM;
    fo.kernel_clears = true;
    et::AdamPack ap{};
    for (int t = 0; t < ntables; ++t) {
        const et_adam_desc& d = ad[t];
        ap.v[t] = d.v;
        ap.ld_v[t] = d.ld_v;
        ap.step[t] = d.step;
        if (et::ada_work(ag[t])) ap.work |= 1u << t;
        const bool v_vec = rowwise ? ((uintptr_t)d.v & 3u) == 0
                                   : et::aligned16(d.v) && d.ld_v % 4 == 0;
        if (!v_vec) fo.no_vec |= 1u << t;
    }
    rc = et::pack_adagrad_tables(dtype, ag, ntables, false, stream, run, fo);
    if (rc != ET_OK) return rc;
    ap.ragged = run.ap.ragged;
    et::UpdatePack mpack = run.pack, wpack = run.pack;  // idx: the first moment / the weights
    bool weighted = false;
    for (int t = 0; t < ntables; ++t) {
        const void* w = et::ada_work(ag[t]) ? descs[t].weights : nullptr;
        mpack.d[t].idx = static_cast<const int64_t*>(ad[t].m);
        mpack.d[t].ld_idx = ad[t].ld_m;
        wpack.d[t].idx = static_cast<const int64_t*>(w);
        weighted = weighted || w != nullptr;
    }
    return et::dispatch_adagrad(dtype, flags, [&](auto e, auto row, auto nt) {
        using T = typename decltype(e)::type;
        using C = typename decltype(e)::acc;
        constexpr bool ROW = decltype(row)::value, NT = decltype(nt)::value;
        const et::AdamHyper<C> h{(C)eta,          (C)eps,          (C)beta1,
                                 (C)beta2,        (C)(1.0 - beta1), (C)(1.0 - beta2)};
        if (!weighted)  // no table carries weights: et_sparse_adam's own launches
            return et::launch_adam<T, C, ROW, NT>(run, mpack, ap, h);
        return et::launch_weighted_adam<T, C, ROW, NT>(run, mpack, wpack, ap, h, pair_ws);
    });
}
