// et_adam.hip — sparse Adam with an element-wise or a row-wise second moment over fixed-pool
// and ragged gradients, textually included by et_update.hip after et_adagrad.hip.  The front
// of the pipeline is AdaGrad's (pack_adagrad_tables: k_ragged_bag_ids, group_occurrences with
// chunk = kChunk) and so is the gradient sum g of a column (ada_occ_sum, the chunk rule);
// the back end is new: a step kernel, a chunk pass and a combine pass that carry two moments
// and the step state beside the table column.
//
// Semantics (include/embtab.h states them in full), in the accumulator type C, every
// operation rounded once (-ffp-contract=off), sqrt and / correctly rounded:
//   step {p1, p2}:  p1' = p1 * b1, p2' = p2 * b2 once per call and table with work;
//                   c1 = 1 - p1', c2 = 1 - p2'
//   m' = (b1 * m) + (omb1 * g)
//   v' = (b2 * v) + (omb2 * (g * g))        row-wise: (omb2 * ((sum_f g_f^2) / dim))
//   w' = T(C(w) - (eta * (m' / c1)) / (sqrt(v' / c2) + eps))
//
// Kernels:
//   k_adam_advance          one small launch in front: the step products of every table with
//                           work.  Not folded into the chunk pass: a chunk record would have to
//                           read p, and whichever lane group wrote p' back would race with the
//                           groups of other workgroups still reading p (no grid-wide order
//                           without a second counter and a spin).  A launch boundary gives every
//                           reader p' for 2 x 32 multiplies.
//   k_adam_chunks<D>        Float32 tables whose rows, gradients and moments are multiples of 16
//                           bytes, dim <= ET_ADAM_VEC_MAX_DIM: the lane-group layout of
//                           k_adagrad_chunks (D/4 lanes per record, at most a wave, capacity
//                           masked below the next power of two).  A single-chunk column issues
//                           its loads of w, m and v (or the scalar v) before the gradient
//                           gather (eight 16-byte loads per lane in flight) and is applied in
//                           place; a chunk of a longer column stores its partial row in C.
//   k_adam_combine<D>       one lane group per multi-chunk column: w, m and v first, then its
//                           partial rows in chunk order, added serially.
//   k_adam_*_generic        every other table (element type, dim, alignment): one wave per
//                           chunk record or multi-chunk column, lanes over features.
// The row-wise sum of squares is reduced inside the lane group with lane shuffles (no LDS, no
// barrier).  Everything runs on the caller's stream, and every node of a captured call is a
// kernel (the front's clears included); nothing synchronises the host.
//
// Where the first moment rides: the kernels get a copy of the UpdatePack whose d[t].idx /
// d[t].ld_idx hold table t's m / ld_m (the key pass is the last reader of idx, as in
// et_weighted_adagrad), so the argument block stays below the 4 KiB of a kernel launch with
// 32 tables; v, ld_v and the step pointers are the AdamPack.

// Every operation of the definition is one scalar IEEE operation: the Adam kernels are
// compiled without the packed fp32 ALU forms (the attribute is a device-side one).
#if defined(__HIP_DEVICE_COMPILE__)
#define ET_ADAM_KERNEL __attribute__((target("no-packed-fp32-ops")))
#else
#define ET_ADAM_KERNEL
#endif

namespace et {

struct AdamPack {
    void* v[ET_MAX_TABLES_PER_LAUNCH];
    int64_t ld_v[ET_MAX_TABLES_PER_LAUNCH];
    void* step[ET_MAX_TABLES_PER_LAUNCH];
    uint32_t ragged;  // bit t: the gradient column of an occurrence is bag_ids[occurrence]
    uint32_t work;    // bit t: the table has work (its step advances)
};

template <typename C>
struct AdamHyper {
    C eta, eps, b1, b2, omb1, omb2;
};

template <typename C>
__device__ __forceinline__ C* adam_m_ptr(const et_update_desc& d, uint32_t row) {
    return reinterpret_cast<C*>(const_cast<int64_t*>(d.idx)) + (uint64_t)row * (uint64_t)d.ld_idx;
}

template <typename C>
__device__ __forceinline__ C adam_m(C m, C g, const AdamHyper<C>& h) {
    return (h.b1 * m) + (h.omb1 * g);
}

template <typename C>
__device__ __forceinline__ C adam_v(C v, C q, const AdamHyper<C>& h) {
    return (h.b2 * v) + (h.omb2 * q);
}

// sqrt(vh) + eps of the bias-corrected second moment
template <typename C>
__device__ __forceinline__ C adam_den(C v2, C c2, C eps) {
    return ada_sqrt(v2 / c2) + eps;
}

// w' = T(C(w) - (eta * mh) / dd): one rounding to T (the barrier as in ada_step).
template <typename T, typename C>
__device__ __forceinline__ T adam_step(T w, C m2, C c1, C dd, C eta) {
    C r = C(w) - (eta * (m2 / c1)) / dd;
    if constexpr (!__is_same(T, C)) asm volatile("" : "+v"(r));
    return (T)r;
}

template <typename C>
__global__ ET_ADAM_KERNEL __launch_bounds__(64) void k_adam_advance(AdamPack ap, int ntables, C b1,
                                                                     C b2) {
    const int t = threadIdx.x;
    if (t >= ntables || !((ap.work >> t) & 1u)) return;
    C* p = reinterpret_cast<C*>(ap.step[t]);
    const C p1 = p[0] * b1, p2 = p[1] * b2;
    p[0] = p1;
    p[1] = p2;
}

// Vector path -------------------------------------------------------------------------------

__device__ __forceinline__ void adam_unpack(const u32x4& a, float (&f)[4]) {
    f[0] = __uint_as_float(a.x), f[1] = __uint_as_float(a.y);
    f[2] = __uint_as_float(a.z), f[3] = __uint_as_float(a.w);
}

__device__ __forceinline__ u32x4 adam_pack(const float (&f)[4]) {
    return u32x4{__float_as_uint(f[0]), __float_as_uint(f[1]), __float_as_uint(f[2]),
                 __float_as_uint(f[3])};
}

// The update of one column from its gradient sum g: x the table column, mo its first moment,
// vo its element-wise second moment (or vrow, its row-wise one), all loaded by the caller.
// All lanes of the group are active (the row-wise reduction shuffles inside the group).
template <int D, bool ROW, bool NT>
__device__ __forceinline__ void adam_apply_row(
    float* __restrict__ w, float* __restrict__ mp, float* __restrict__ vp,
    const u32x4 (&x)[(D / 4 < 64 ? 1 : D / 4 / 64)], const u32x4 (&mo)[(D / 4 < 64 ? 1 : D / 4 / 64)],
    const u32x4 (&vo)[(D / 4 < 64 ? 1 : D / 4 / 64)], float vrow,
    const float (&g)[(D / 4 < 64 ? 1 : D / 4 / 64)][4], int sub, int vpr, int dim, float c1,
    float c2, const AdamHyper<float>& h) {
    constexpr int VPR = D / 4;
    constexpr int LPR = VPR < 64 ? VPR : 64;
    constexpr int NV = VPR / LPR;
    u32x4* wp = reinterpret_cast<u32x4*>(w) + sub;
    u32x4* mq = reinterpret_cast<u32x4*>(mp) + sub;
    float dd = 0.0f;
    if constexpr (ROW) {
        float ss = 0.0f;
#pragma unroll
        for (int v = 0; v < NV; ++v)
            if (sub + v * LPR < vpr) {
#pragma unroll
                for (int e = 0; e < 4; ++e) ss = ss + g[v][e] * g[v][e];
            }
#pragma unroll
        for (int s = LPR / 2; s >= 1; s >>= 1) ss = ss + __shfl_xor(ss, s, 64);
        const float v2 = adam_v(vrow, ss / (float)dim, h);
        dd = adam_den(v2, c2, h.eps);
        if (sub == 0) store_scalar<NT>(vp, v2);
    }
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        float wi[4], mi[4], vi[4], wo[4], m2[4], v2[4];
        adam_unpack(x[v], wi);
        adam_unpack(mo[v], mi);
        if constexpr (!ROW) adam_unpack(vo[v], vi);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            m2[e] = adam_m(mi[e], g[v][e], h);
            float de = dd;
            if constexpr (!ROW) {
                v2[e] = adam_v(vi[e], g[v][e] * g[v][e], h);
                de = adam_den(v2[e], c2, h.eps);
            }
            wo[e] = adam_step<float, float>(wi[e], m2[e], c1, de, h.eta);
        }
        if (sub + v * LPR < vpr) {
            store16<NT>(mq + v * LPR, adam_pack(m2));
            if constexpr (!ROW)
                store16<NT>(reinterpret_cast<u32x4*>(vp) + sub + v * LPR, adam_pack(v2));
            store16<NT>(wp + v * LPR, adam_pack(wo));
        }
    }
}

// Chunk pass: lane group q of the grid takes chunk records q, q + groups, ...
template <int D, bool ROW, bool NT>
__global__ ET_ADAM_KERNEL __launch_bounds__(256) void k_adam_chunks(
    UpdatePack pack, AdamPack ap, int ntables, const uint32_t* __restrict__ vals,
    const ChunkRec* __restrict__ recs, const uint32_t* __restrict__ counters,
    const uint32_t* __restrict__ bag_ids, float* __restrict__ partials,
    uint32_t* __restrict__ pany, int pdim, uint32_t sent, AdamHyper<float> h, uint32_t my_mask) {
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
        const bool any = ada_occ_sum<D, U>(reinterpret_cast<const float*>(d.delta),
                                           (uint64_t)d.ld_delta, pack.occ_off[t], (uint32_t)d.pool,
                                           (ap.ragged >> t) & 1u, bag_ids, vals, r.s0, r.s1, g, sub,
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

// Combine pass: lane group q takes the multi-chunk columns q, q + groups, ... of the list.
template <int D, bool ROW, bool NT>
__global__ ET_ADAM_KERNEL __launch_bounds__(256) void k_adam_combine(
    UpdatePack pack, AdamPack ap, int ntables, const uint32_t* __restrict__ keys,
    const uint32_t* __restrict__ seg_start, const uint32_t* __restrict__ partial_start,
    const uint32_t* __restrict__ counters, const uint32_t* __restrict__ mlist,
    const float* __restrict__ partials, const uint32_t* __restrict__ pany, int pdim, uint32_t sent,
    AdamHyper<float> h, uint32_t my_mask) {
    constexpr int VPR = D / 4;
    constexpr int LPR = VPR < 64 ? VPR : 64;
    constexpr int NV = VPR / LPR;
    constexpr int GPW = 64 / LPR;
    constexpr int U = NV >= 8 ? 1 : 8 / NV;
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
        float* mp = adam_m_ptr<float>(d, row);
        float* vp = reinterpret_cast<float*>(ap.v[t]) +
                    (ROW ? (uint64_t)row : (uint64_t)row * (uint64_t)ap.ld_v[t]);
        const int vpr = d.dim / 4;
        int vix[NV];
        vec_index<LPR, NV>(sub, vpr, vix);
        u32x4 x[NV], mo[NV], vo[NV];
        float vrow = 0.0f;
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            x[v] = reinterpret_cast<const u32x4*>(w)[vix[v]];
            mo[v] = reinterpret_cast<const u32x4*>(mp)[vix[v]];
            vo[v] = u32x4{0u, 0u, 0u, 0u};
        }
        if constexpr (ROW) {
            vrow = *vp;
        } else {
#pragma unroll
            for (int v = 0; v < NV; ++v) vo[v] = reinterpret_cast<const u32x4*>(vp)[vix[v]];
        }
        const float* st = reinterpret_cast<const float*>(ap.step[t]);
        const float c1 = 1.0f - st[0], c2 = 1.0f - st[1];
        const uint32_t p0 = partial_start[seg], np = partial_start[seg + 1] - p0;
        float acc[NV][4];
        uint32_t any = pany[p0];
        {
            const u32x4* pp = reinterpret_cast<const u32x4*>(partials + (uint64_t)p0 * pdim);
#pragma unroll
            for (int v = 0; v < NV; ++v) adam_unpack(pp[vix[v]], acc[v]);
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
        if (any)
            adam_apply_row<D, ROW, NT>(w, mp, vp, x, mo, vo, vrow, acc, sub, vpr, d.dim, c1, c2, h);
    }
}

// Generic path ------------------------------------------------------------------------------
// One wave per chunk record or multi-chunk column; lane l holds features f0 + l + 64 k,
// k < kAdaK, of the block of 64 * kAdaK features at f0, as in ada_apply_generic.
// sum_block(f0, acc) fills the block's gradient sums and returns whether any occurrence took
// part (wave-uniform).
template <typename T, typename C, bool ROW, bool NT, typename F>
__device__ __forceinline__ void adam_apply_generic(T* __restrict__ w, C* __restrict__ mp,
                                                   C* __restrict__ vp, int dim, int lane, C c1,
                                                   C c2, const AdamHyper<C>& h, F&& sum_block) {
    C acc[kAdaK];
    const bool one = dim <= 64 * kAdaK;
    C v2r = C(0), dd = C(0);
    if constexpr (ROW) {
        // the sum of squares needs every feature before the first one is applied: a row of
        // more than 64 * kAdaK features forms its gradient sums twice
        C ss = C(0);
        for (int f0 = 0; f0 < dim; f0 += 64 * kAdaK) {
            if (!sum_block(f0, acc)) return;
#pragma unroll
            for (int k = 0; k < kAdaK; ++k)
                if (f0 + lane + 64 * k < dim) ss = ss + acc[k] * acc[k];
        }
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) ss = ss + __shfl_xor(ss, s, 64);
        v2r = adam_v(*vp, ss / C(dim), h);
        dd = adam_den(v2r, c2, h.eps);
    }
    for (int f0 = 0; f0 < dim; f0 += 64 * kAdaK) {
        if (!(ROW && one))
            if (!sum_block(f0, acc)) return;
#pragma unroll
        for (int k = 0; k < kAdaK; ++k) {
            const int f = f0 + lane + 64 * k;
            if (f >= dim) continue;
            const C m2 = adam_m(mp[f], acc[k], h);
            C de = dd;
            if constexpr (!ROW) {
                const C v2 = adam_v(vp[f], acc[k] * acc[k], h);
                de = adam_den(v2, c2, h.eps);
                store_scalar<NT>(vp + f, v2);
            }
            store_scalar<NT>(mp + f, m2);
            store_scalar<NT>(w + f, adam_step<T, C>(w[f], m2, c1, de, h.eta));
        }
    }
    if constexpr (ROW)
        if (lane == 0) store_scalar<NT>(vp, v2r);
}

// The gradient sums of features f0 + lane + 64 k over sorted occurrences [s0, s1), kAdaE
// gradient rows in flight.
template <typename T, typename C>
__device__ __forceinline__ bool adam_occ_block(const T* __restrict__ delta, uint64_t ldd, int dim,
                                               bool ragged, uint32_t occ_off, uint32_t pool,
                                               const uint32_t* __restrict__ bag_ids,
                                               const uint32_t* __restrict__ vals, uint32_t s0,
                                               uint32_t s1, int lane, int f0, C (&acc)[kAdaK]) {
#pragma unroll
    for (int k = 0; k < kAdaK; ++k) acc[k] = C(0);
    bool any = false;
    for (uint32_t e0 = s0; e0 < s1; e0 += 64) {
        const uint32_t cnt = s1 - e0 < 64u ? s1 - e0 : 64u;
        uint32_t myb = 0;
        if ((uint32_t)lane < cnt)
            myb = ada_bag(vals[e0 + (uint32_t)lane], ragged, occ_off, pool, bag_ids);
        for (uint32_t j0 = 0; j0 < cnt; j0 += kAdaE) {
            uint32_t b[kAdaE];  // 0 beyond the chunk (lanes >= cnt hold 0)
#pragma unroll
            for (int j = 0; j < kAdaE; ++j) {
                const uint32_t src = j0 + j;
                b[j] = src < 64u ? (uint32_t)__shfl((int)myb, (int)src, 64) : 0u;
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
                for (int k = 0; k < kAdaK; ++k) acc[k] = acc[k] + C(x[j][k]);
            }
        }
    }
    return any;
}

// The same block from the np partial rows of a multi-chunk column, in chunk order.
template <typename C>
__device__ __forceinline__ bool adam_partial_block(const C* __restrict__ partials,
                                                   const uint32_t* __restrict__ pany, int pdim,
                                                   int dim, uint32_t p0, uint32_t np, int lane,
                                                   int f0, C (&acc)[kAdaK]) {
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
}

// G is the gradient's element type, as in k_adagrad_chunks_generic.
template <typename T, typename C, bool ROW, bool NT, typename G = T>
__global__ ET_ADAM_KERNEL __launch_bounds__(256) void k_adam_chunks_generic(
    UpdatePack pack, AdamPack ap, int ntables, const uint32_t* __restrict__ vals,
    const ChunkRec* __restrict__ recs, const uint32_t* __restrict__ counters,
    const uint32_t* __restrict__ bag_ids, C* __restrict__ partials, uint32_t* __restrict__ pany,
    int pdim, uint32_t sent, AdamHyper<C> h) {
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
        const G* __restrict__ delta = reinterpret_cast<const G*>(d.delta);
        const uint64_t ldd = (uint64_t)d.ld_delta;
        const bool ragged = (ap.ragged >> t) & 1u;
        const uint32_t occ_off = pack.occ_off[t], pool = (uint32_t)d.pool;
        const uint32_t s0 = r.s0, s1 = r.s1;
        auto sum_block = [&](int f0, C(&acc)[kAdaK]) __attribute__((always_inline)) -> bool {
            return adam_occ_block<G, C>(delta, ldd, dim, ragged, occ_off, pool, bag_ids, vals, s0,
                                        s1, lane, f0, acc);
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

template <typename T, typename C, bool ROW, bool NT>
__global__ ET_ADAM_KERNEL __launch_bounds__(256) void k_adam_combine_generic(
    UpdatePack pack, AdamPack ap, int ntables, const uint32_t* __restrict__ keys,
    const uint32_t* __restrict__ seg_start, const uint32_t* __restrict__ partial_start,
    const uint32_t* __restrict__ counters, const uint32_t* __restrict__ mlist,
    const C* __restrict__ partials, const uint32_t* __restrict__ pany, int pdim, uint32_t sent,
    AdamHyper<C> h) {
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
        auto sum_block = [&](int f0, C(&acc)[kAdaK]) __attribute__((always_inline)) -> bool {
            return adam_partial_block<C>(partials, pany, pdim, dim, p0, np, lane, f0, acc);
        };
        const uint32_t row = key - pack.row_off[t];
        T* w = col_ptr<T>(d.table, d.ld_table, d.cols_per_page, row);
        C* vp = reinterpret_cast<C*>(ap.v[t]) +
                (ROW ? (uint64_t)row : (uint64_t)row * (uint64_t)ap.ld_v[t]);
        const C* st = reinterpret_cast<const C*>(ap.step[t]);
        adam_apply_generic<T, C, ROW, NT>(w, adam_m_ptr<C>(d, row), vp, dim, lane, C(1) - st[0],
                                          C(1) - st[1], h, sum_block);
    }
}

// Host --------------------------------------------------------------------------------------

inline et_adagrad_desc adam_as_adagrad(const et_adam_desc& d) {
    // the shared front validates, sizes and packs these: the first moment as the state
    return et_adagrad_desc{d.table, d.ld_table, d.nrows,         d.dim,    d.pool,
                           d.delta, d.ld_delta, d.idx,           d.ld_idx, d.batch,
                           d.cols_per_page,     d.colptr, d.nnz, d.m,      d.ld_m};
}

inline int adam_table_count(const et_adam_desc* descs, int ntables) {
    if (ntables < 0) return fail(ET_ERR_ARG, "negative ntables");
    if (ntables > ET_MAX_TABLES_PER_LAUNCH)
        return fail(ET_ERR_ARG, "at most %d tables per update call", ET_MAX_TABLES_PER_LAUNCH);
    if (ntables > 0 && !descs) return fail(ET_ERR_ARG, "descs is NULL");
    return ET_OK;
}

// The checks AdaGrad's validation (run first, on the first moment) does not make: v and step,
// and every moment and step block against every other block of the call.
inline int validate_adam_blocks(int dtype, const et_adam_desc* descs, int ntables, bool rowwise) {
    struct Block {
        uintptr_t a;
        uint64_t n;
        int t;
        const char* what;
    };
    static const char* const kTable = "the table";
    static const char* const kStep = "step";
    Block blk[4 * ET_MAX_TABLES_PER_LAUNCH];
    int nb = 0;
    const uint64_t es = (uint64_t)elsize(dtype), cs = dtype == ET_F64 ? 8u : 4u;
    for (int t = 0; t < ntables; ++t) {
        const et_adam_desc& d = descs[t];
        if (!ada_work(adam_as_adagrad(d))) continue;
        if (!d.v) return fail(ET_ERR_ARG, "table %d: v is NULL", t);
        if (!d.step) return fail(ET_ERR_ARG, "table %d: step is NULL", t);
        if (!rowwise && d.ld_v < d.dim) return fail(ET_ERR_ARG, "table %d: ld_v < dim", t);
        blk[nb++] = Block{(uintptr_t)d.step, 2 * cs, t, kStep};
        if (d.nrows == 0) continue;
        const uint64_t rows1 = (uint64_t)(d.nrows - 1), dim = (uint64_t)d.dim;
        // a paged table is its array of page pointers here (the pages are device data)
        const uint64_t tbytes =
            d.cols_per_page > 0
                ? (uint64_t)((d.nrows + d.cols_per_page - 1) / d.cols_per_page) * 8u
                : (rows1 * (uint64_t)d.ld_table + dim) * es;
        blk[nb++] = Block{(uintptr_t)d.table, tbytes, t, kTable};
        blk[nb++] = Block{(uintptr_t)d.m, (rows1 * (uint64_t)d.ld_m + dim) * cs, t, "m"};
        blk[nb++] = Block{(uintptr_t)d.v,
                          rowwise ? (uint64_t)d.nrows * cs : (rows1 * (uint64_t)d.ld_v + dim) * cs,
                          t, "v"};
    }
    for (int i = 0; i < nb; ++i)
        for (int j = i + 1; j < nb; ++j) {
            const Block &a = blk[i], &b = blk[j];
            if (a.what == kTable && b.what == kTable) continue;  // not this call's business
            if (a.what == kStep && b.what == kStep && a.a == b.a)
                return fail(ET_ERR_ARG, "tables %d and %d name the same step", a.t, b.t);
            if (ranges_overlap(a.a, a.n, b.a, b.n))
                return fail(ET_ERR_ARG, "%s of table %d overlaps %s of table %d", b.what, b.t,
                            a.what, a.t);
        }
    return ET_OK;
}

constexpr uint32_t kAdamFlags = ET_FLAG_NONTEMPORAL | ET_FLAG_ADAM_ROWWISE;

// `known`: flags beyond kAdamFlags this entry takes (kDeltaFlags for et_sparse_adam).
inline int check_adam_call(int dtype, uint32_t flags, double beta1, double beta2,
                           uint32_t known = 0) {
    if (dtype != ET_F32 && dtype != ET_F64 && dtype != ET_F16 && dtype != ET_BF16)
        return fail(ET_ERR_UNSUPPORTED, "sparse Adam: dtype %d", dtype);
    if (flags & kAdaSgdOnly)
        return fail(ET_ERR_UNSUPPORTED, "sparse Adam: flags 0x%x belong to the SGD",
                    flags & kAdaSgdOnly);
    if (flags & ~(kAdamFlags | known))
        return fail(ET_ERR_ARG, "sparse Adam: unknown flags 0x%x", flags & ~(kAdamFlags | known));
    if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0))
        return fail(ET_ERR_ARG, "sparse Adam: beta (%g, %g) outside [0, 1)", beta1, beta2);
    return check_delta_flags("sparse Adam", dtype, flags & known);
}

template <typename F>
void with_adam_capacity(int cap, F&& f) {
    static_assert(ET_ADAM_VEC_MAX_DIM == 1024, "the capacities of the Adam vector kernels");
    with_capacity_in<16, 32, 64, 128, 256, 512, 1024>(cap, f);
}

template <typename T, typename C, bool ROW, bool NT>
int launch_adam(const AdaRun& r, const UpdatePack& mpack, const AdamPack& ap, AdamHyper<C> h) {
    hipLaunchKernelGGL((k_adam_advance<C>), dim3(1), dim3(64), 0, r.s, ap, r.ntables, h.b1, h.b2);
    ET_LAUNCH_CHECK("k_adam_advance");
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
                hipLaunchKernelGGL((k_adam_chunks<D, ROW, NT>), dim3(grid), dim3(256), 0, r.s,
                                   mpack, ap, r.ntables, r.gr.vals, u.recs, u.counters, r.w.bag,
                                   partials, r.w.pany, r.pdim, r.sent, h, r.vg.mask[i]);
                hipLaunchKernelGGL((k_adam_combine<D, ROW, NT>),
                                   dim3((unsigned)(cb < 2048 ? cb : 2048)), dim3(256), 0, r.s,
                                   mpack, ap, r.ntables, r.gr.keys, u.seg_start, u.multi,
                                   u.counters, u.mlist, partials, r.w.pany, r.pdim, r.sent, h,
                                   r.vg.mask[i]);
            });
        ET_LAUNCH_CHECK("k_adam_chunks");
    }
    if (r.any_generic) {
        C* partials = reinterpret_cast<C*>(r.w.partials);
        const int64_t cb = cdiv64(mmax, 4);
        hipLaunchKernelGGL((k_adam_chunks_generic<T, C, ROW, NT>), dim3(grid), dim3(256), 0, r.s,
                           mpack, ap, r.ntables, r.gr.vals, u.recs, u.counters, r.w.bag, partials,
                           r.w.pany, r.pdim, r.sent, h);
        hipLaunchKernelGGL((k_adam_combine_generic<T, C, ROW, NT>),
                           dim3((unsigned)(cb < 4096 ? cb : 4096)), dim3(256), 0, r.s, mpack, ap,
                           r.ntables, r.gr.keys, u.seg_start, u.multi, u.counters, u.mlist,
                           partials, r.w.pany, r.pdim, r.sent, h);
        ET_LAUNCH_CHECK("k_adam_chunks_generic");
    }
    return ET_OK;
}

// et_mixed_grad.hip: the advance, chunk and combine passes of a call with a 16-bit gradient.
inline int launch_adam_mixed(const AdaRun& r, const UpdatePack& mpack, const AdamPack& ap,
                             const AdamHyper<float>& h, uint32_t flags);

}  // namespace et

extern "C" int et_adam_workspace_size(const et_adam_desc* descs, int32_t ntables,
                                      int64_t* bytes) {
    et::clear_err();
    if (!bytes) return et::fail(ET_ERR_ARG, "bytes is NULL");
    int rc = et::adam_table_count(descs, ntables);
    if (rc != ET_OK) return rc;
    et_adagrad_desc ad[ET_MAX_TABLES_PER_LAUNCH];
    for (int t = 0; t < ntables; ++t) ad[t] = et::adam_as_adagrad(descs[t]);
    int64_t n;
    int pdim;
    // sized for either form and any float type: only the sizes are read
    rc = et::validate_adagrad(ET_F32, ad, ntables, true, &n, &pdim, false);
    if (rc != ET_OK) return rc;
    *bytes = et::carve_adagrad_ws(nullptr, n, pdim).bytes;
    return ET_OK;
}

extern "C" int et_sparse_adam(int dtype, const et_adam_desc* descs, int32_t ntables, double eta,
                              double beta1, double beta2, double eps, uint32_t flags,
                              void* workspace, int64_t ws_bytes, void* stream) {
    et::clear_err();
    int rc = et::check_adam_call(dtype, flags, beta1, beta2, et::kDeltaFlags);
    if (rc != ET_OK) return rc;
    rc = et::adam_table_count(descs, ntables);
    if (rc != ET_OK) return rc;
    const bool rowwise = (flags & ET_FLAG_ADAM_ROWWISE) != 0;
    et_adagrad_desc ad[ET_MAX_TABLES_PER_LAUNCH];
    for (int t = 0; t < ntables; ++t) ad[t] = et::adam_as_adagrad(descs[t]);
    et::AdaRun run;
    // the first moment is always element-wise: AdaGrad's checks of an element-wise state
    rc = et::validate_adagrad(dtype, ad, ntables, false, &run.n, &run.pdim, true, "m");
    if (rc != ET_OK) return rc;
    rc = et::validate_adam_blocks(dtype, descs, ntables, rowwise);
    if (rc != ET_OK || run.n == 0) return rc;
    run.w = et::carve_adagrad_ws(static_cast<char*>(workspace), run.n, run.pdim);
    if (!workspace || ws_bytes < run.w.bytes)
        return et::fail(ET_ERR_WORKSPACE, "workspace of %lld bytes needed",
                        (long long)run.w.bytes);
    et::AdaFrontOpts fo;
    fo.vec_max_dim = ET_ADAM_VEC_MAX_DIM;
    fo.kernel_clears = true;
    fo.delta16 = (flags & et::kDeltaFlags) != 0;
    et::AdamPack ap{};
    for (int t = 0; t < ntables; ++t) {
        const et_adam_desc& d = descs[t];
        ap.v[t] = d.v;
        ap.ld_v[t] = d.ld_v;
        ap.step[t] = d.step;
        if (et::ada_work(ad[t])) ap.work |= 1u << t;
        const bool v_vec = rowwise ? ((uintptr_t)d.v & 3u) == 0
                                   : et::aligned16(d.v) && d.ld_v % 4 == 0;
        if (!v_vec) fo.no_vec |= 1u << t;
    }
    rc = et::pack_adagrad_tables(dtype, ad, ntables, false, stream, run, fo);
    if (rc != ET_OK) return rc;
    ap.ragged = run.ap.ragged;
    et::UpdatePack mpack = run.pack;  // idx / ld_idx: the first moment (see the file comment)
    for (int t = 0; t < ntables; ++t) {
        mpack.d[t].idx = static_cast<const int64_t*>(descs[t].m);
        mpack.d[t].ld_idx = descs[t].ld_m;
    }
    if (fo.delta16) {
        const et::AdamHyper<float> h{(float)eta,   (float)eps,           (float)beta1,
                                     (float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2)};
        return et::launch_adam_mixed(run, mpack, ap, h, flags);
    }
    return et::dispatch_adagrad(dtype, flags, [&](auto e, auto row, auto nt) {
        using T = typename decltype(e)::type;
        using C = typename decltype(e)::acc;
        const et::AdamHyper<C> h{(C)eta,          (C)eps,          (C)beta1,
                                 (C)beta2,        (C)(1.0 - beta1), (C)(1.0 - beta2)};
        return et::launch_adam<T, C, decltype(row)::value, decltype(nt)::value>(run, mpack, ap, h);
    });
}
