// et_adagrad.hip — sparse AdaGrad (element-wise and row-wise) over fixed-pool and ragged
// gradients, textually included by et_update.hip.  The front of the pipeline is
// group_occurrences unchanged with chunk = kChunk: a ragged table goes in as a vector index
// (pool = 1) plus the bag id of every entry (k_ragged_bag_ids), as in et_ragged_sgd, so both
// kinds ride in one call.  The back end is new: a chunk pass and a combine pass that carry the
// optimiser state beside the table column.
//
// Semantics (include/embtab.h states them in full; the reference has no AdaGrad): per
// distinct column with a participating occurrence, in the accumulator type C (float, or
// double for Float64 tables):
//   p_c = +0; p_c += delta[:, bag] for the occurrences of chunk c (kChunk list positions each)
//   g   = p_0                       one chunk
//       = ((p_0 + p_1) + p_2) + ... in chunk order, serially, otherwise
//   element-wise: s' = s + g*g                  row-wise: s' = s + (sum_f g_f^2) / dim
//   d = sqrt(s') + eps ;  w' = T(C(w) - (eta*g)/d)
// every operation rounded once in C (-ffp-contract=off), sqrt and / correctly rounded.
// A ragged entry of the capacity tail (bag id 0) adds nothing but keeps its list position, so
// the rounding of a column of more than kChunk entries depends on what sits in the tail.
//
// Kernels:
//   k_adagrad_chunks<D>     Float32 tables whose rows are a multiple of 16 bytes (capacity D =
//                           the power of two at or above dim, masked below it, up to 2048):
//                           one lane group of D/4 lanes (at most a wave) per chunk record.  A
//                           single-chunk column loads its table column and state first, then
//                           gathers its gradient rows (eight 16-byte loads per lane in flight:
//                           eight rows up to dim 256) and is applied in place; a chunk of a
//                           longer column stores its partial row in C.
//   k_adagrad_combine<D>    one lane group per multi-chunk column: its partial rows in chunk
//                           order, sixteen 16-byte loads per lane in flight, added serially.
//   k_adagrad_*_generic     every other table (element type, dim, alignment): one wave per
//                           chunk record or multi-chunk column, lanes over features.
// The row-wise sum of squares is reduced inside the lane group with lane shuffles (no LDS,
// no barrier).  Everything runs on the caller's stream; nothing synchronises the host.

namespace et {

struct AdaPack {
    void* state[ET_MAX_TABLES_PER_LAUNCH];
    int64_t ld_state[ET_MAX_TABLES_PER_LAUNCH];
    uint32_t ragged;  // bit t: the gradient column of an occurrence is bag_ids[occurrence]
};

template <typename C>
__device__ __forceinline__ C ada_sqrt(C x) {
    if constexpr (__is_same(C, double))
        return __builtin_sqrt(x);
    else
        return __builtin_sqrtf(x);
}

// w' = T(C(w) - (eta*g)/d): one rounding to T.  The barrier keeps the fp32 result in a
// register of its own, so no mixed-precision instruction can round it straight to half.
template <typename T, typename C>
__device__ __forceinline__ T ada_step(T w, C g, C d, C eta) {
    C r = C(w) - (eta * g) / d;
    if constexpr (!__is_same(T, C)) asm volatile("" : "+v"(r));
    return (T)r;
}

// 1-based gradient column of sorted occurrence `o` of table t, 0 for a ragged entry of the
// capacity tail.
__device__ __forceinline__ uint32_t ada_bag(uint32_t o, bool ragged, uint32_t occ_off,
                                            uint32_t pool,
                                            const uint32_t* __restrict__ bag_ids) {
    return ragged ? bag_ids[o] : (o - occ_off) / pool + 1u;
}

// Vector path -------------------------------------------------------------------------------

// acc += delta[:, bag] over sorted occurrences [s0, s1) in order (one lane group).  The group
// reads LPR occurrence ids at once, turns them into gradient columns and hands them out with
// a lane shuffle; U gradient rows are loaded before the first add.  Control flow is uniform
// inside a lane group, not inside a wave (the groups of a wave walk different chunks).
// Returns whether any occurrence took part.
template <int D, int U>
__device__ __forceinline__ bool ada_occ_sum(const float* __restrict__ delta, uint64_t ldd,
                                            uint32_t occ_off, uint32_t pool, bool ragged,
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
        if (sub < cnt) myb = ada_bag(vals[c0 + (uint32_t)sub], ragged, occ_off, pool, bag_ids);
        for (int i0 = 0; i0 < cnt; i0 += U) {
            uint32_t b[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int j = i0 + u;
                const uint32_t v = (uint32_t)__shfl((int)myb, g * LPR + (j < LPR ? j : LPR - 1), 64);
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
                if (b[u] == 0u) continue;  // past the chunk, or the capacity tail
                any = true;
#pragma unroll
                for (int v = 0; v < NV; ++v) {
                    acc[v][0] = acc[v][0] + __uint_as_float(buf[u][v].x);
                    acc[v][1] = acc[v][1] + __uint_as_float(buf[u][v].y);
                    acc[v][2] = acc[v][2] + __uint_as_float(buf[u][v].z);
                    acc[v][3] = acc[v][3] + __uint_as_float(buf[u][v].w);
                }
            }
        }
    }
    return any;
}

// The update of one column from its gradient sum g: x the table column, st its element-wise
// state (or srow, its row-wise state), both loaded by the caller.  All lanes of the group
// are active (the row-wise reduction shuffles inside the group).
template <int D, bool ROW, bool NT>
__device__ __forceinline__ void ada_apply_row(
    float* __restrict__ w, float* __restrict__ sp, const u32x4 (&x)[(D / 4 < 64 ? 1 : D / 4 / 64)],
    const u32x4 (&st)[(D / 4 < 64 ? 1 : D / 4 / 64)], float srow,
    const float (&g)[(D / 4 < 64 ? 1 : D / 4 / 64)][4], int sub, int vpr, int dim, float eta,
    float eps) {
    constexpr int VPR = D / 4;
    constexpr int LPR = VPR < 64 ? VPR : 64;
    constexpr int NV = VPR / LPR;
    u32x4* wp = reinterpret_cast<u32x4*>(w) + sub;
    if constexpr (ROW) {
        float ss = 0.0f;
#pragma unroll
        for (int v = 0; v < NV; ++v)
            if (sub + v * LPR < vpr) {
#pragma unroll
                for (int e = 0; e < 4; ++e) ss = ss + g[v][e] * g[v][e];
            }
#pragma unroll
        for (int m = LPR / 2; m >= 1; m >>= 1) ss = ss + __shfl_xor(ss, m, 64);
        const float s2 = srow + ss / (float)dim;
        const float dd = ada_sqrt(s2) + eps;
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            u32x4 y;
            y.x = __float_as_uint(ada_step<float, float>(__uint_as_float(x[v].x), g[v][0], dd, eta));
            y.y = __float_as_uint(ada_step<float, float>(__uint_as_float(x[v].y), g[v][1], dd, eta));
            y.z = __float_as_uint(ada_step<float, float>(__uint_as_float(x[v].z), g[v][2], dd, eta));
            y.w = __float_as_uint(ada_step<float, float>(__uint_as_float(x[v].w), g[v][3], dd, eta));
            if (sub + v * LPR < vpr) store16<NT>(wp + v * LPR, y);
        }
        if (sub == 0) store_scalar<NT>(sp, s2);
    } else {
        u32x4* sq = reinterpret_cast<u32x4*>(sp) + sub;
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            const float wi[4] = {__uint_as_float(x[v].x), __uint_as_float(x[v].y),
                                 __uint_as_float(x[v].z), __uint_as_float(x[v].w)};
            const float si[4] = {__uint_as_float(st[v].x), __uint_as_float(st[v].y),
                                 __uint_as_float(st[v].z), __uint_as_float(st[v].w)};
            float wo[4], so[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                so[e] = si[e] + g[v][e] * g[v][e];
                wo[e] = ada_step<float, float>(wi[e], g[v][e], ada_sqrt(so[e]) + eps, eta);
            }
            if (sub + v * LPR < vpr) {
                store16<NT>(sq + v * LPR, u32x4{__float_as_uint(so[0]), __float_as_uint(so[1]),
                                                __float_as_uint(so[2]), __float_as_uint(so[3])});
                store16<NT>(wp + v * LPR, u32x4{__float_as_uint(wo[0]), __float_as_uint(wo[1]),
                                                __float_as_uint(wo[2]), __float_as_uint(wo[3])});
            }
        }
    }
}

// Chunk pass: lane group q of the grid takes chunk records q, q + groups, ...
template <int D, bool ROW, bool NT>
__global__ __launch_bounds__(256) void k_adagrad_chunks(
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
        const bool any = ada_occ_sum<D, U>(reinterpret_cast<const float*>(d.delta),
                                           (uint64_t)d.ld_delta, pack.occ_off[t], (uint32_t)d.pool,
                                           (ap.ragged >> t) & 1u, bag_ids, vals, r.s0, r.s1, g, sub,
                                           vpr, acc);
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

// Combine pass: lane group q takes the multi-chunk columns q, q + groups, ... of the list.
template <int D, bool ROW, bool NT>
__global__ __launch_bounds__(256) void k_adagrad_combine(
    UpdatePack pack, AdaPack ap, int ntables, const uint32_t* __restrict__ keys,
    const uint32_t* __restrict__ seg_start, const uint32_t* __restrict__ partial_start,
    const uint32_t* __restrict__ counters, const uint32_t* __restrict__ mlist,
    const float* __restrict__ partials, const uint32_t* __restrict__ pany, int pdim, uint32_t sent,
    float eta, float eps, uint32_t my_mask) {
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
        float* sp = reinterpret_cast<float*>(ap.state[t]) +
                    (ROW ? (uint64_t)row : (uint64_t)row * (uint64_t)ap.ld_state[t]);
        const int vpr = d.dim / 4;
        int vix[NV];
        vec_index<LPR, NV>(sub, vpr, vix);
        u32x4 x[NV], st[NV];
        float srow = 0.0f;
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            x[v] = reinterpret_cast<const u32x4*>(w)[vix[v]];
            st[v] = u32x4{0u, 0u, 0u, 0u};
        }
        if constexpr (ROW) {
            srow = *sp;
        } else {
#pragma unroll
            for (int v = 0; v < NV; ++v) st[v] = reinterpret_cast<const u32x4*>(sp)[vix[v]];
        }
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
        if (any) ada_apply_row<D, ROW, NT>(w, sp, x, st, srow, acc, sub, vpr, d.dim, eta, eps);
    }
}

// Generic path ------------------------------------------------------------------------------
// One wave per chunk record or multi-chunk column; lane l holds features f0 + l + 64 k,
// k < kAdaK, of the block of 64 * kAdaK features at f0.  sum_block(f0, acc) fills the block's
// gradient sums and returns whether any occurrence took part (wave-uniform).
constexpr int kAdaK = 4, kAdaE = 8;

template <typename T, typename C, bool ROW, bool NT, typename F>
__device__ __forceinline__ void ada_apply_generic(T* __restrict__ w, C* __restrict__ sp, int dim,
                                                  int lane, C eta, C eps, F&& sum_block) {
    C acc[kAdaK];
    const bool one = dim <= 64 * kAdaK;
    C s2 = C(0), dd = C(0);
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
        for (int m = 32; m >= 1; m >>= 1) ss = ss + __shfl_xor(ss, m, 64);
        s2 = *sp + ss / C(dim);
        dd = ada_sqrt(s2) + eps;
    }
    for (int f0 = 0; f0 < dim; f0 += 64 * kAdaK) {
        if (!(ROW && one))
            if (!sum_block(f0, acc)) return;
#pragma unroll
        for (int k = 0; k < kAdaK; ++k) {
            const int f = f0 + lane + 64 * k;
            if (f >= dim) continue;
            if constexpr (ROW) {
                store_scalar<NT>(w + f, ada_step<T, C>(w[f], acc[k], dd, eta));
            } else {
                const C so = sp[f] + acc[k] * acc[k];
                store_scalar<NT>(sp + f, so);
                store_scalar<NT>(w + f, ada_step<T, C>(w[f], acc[k], ada_sqrt(so) + eps, eta));
            }
        }
    }
    if constexpr (ROW)
        if (lane == 0) store_scalar<NT>(sp, s2);
}

template <typename T, typename C, bool ROW, bool NT>
__global__ __launch_bounds__(256) void k_adagrad_chunks_generic(
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
                if ((uint32_t)lane < cnt)
                    myb = ada_bag(vals[e0 + (uint32_t)lane], ragged, occ_off, pool, bag_ids);
                for (uint32_t j0 = 0; j0 < cnt; j0 += kAdaE) {
                    uint32_t b[kAdaE];  // 0 beyond the chunk (lanes >= cnt hold 0)
#pragma unroll
                    for (int j = 0; j < kAdaE; ++j)
                        b[j] = (uint32_t)__shfl((int)myb, (int)(j0 + j), 64);
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
                        for (int k = 0; k < kAdaK; ++k) acc[k] = acc[k] + C(x[j][k]);
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

template <typename T, typename C, bool ROW, bool NT>
__global__ __launch_bounds__(256) void k_adagrad_combine_generic(
    UpdatePack pack, AdaPack ap, int ntables, const uint32_t* __restrict__ keys,
    const uint32_t* __restrict__ seg_start, const uint32_t* __restrict__ partial_start,
    const uint32_t* __restrict__ counters, const uint32_t* __restrict__ mlist,
    const C* __restrict__ partials, const uint32_t* __restrict__ pany, int pdim, uint32_t sent,
    C eta, C eps) {
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
        const uint32_t row = key - pack.row_off[t];
        T* w = col_ptr<T>(d.table, d.ld_table, d.cols_per_page, row);
        C* sp = reinterpret_cast<C*>(ap.state[t]) +
                (ROW ? (uint64_t)row : (uint64_t)row * (uint64_t)ap.ld_state[t]);
        ada_apply_generic<T, C, ROW, NT>(w, sp, dim, lane, eta, eps, sum_block);
    }
}

// Host --------------------------------------------------------------------------------------

struct AdaWs {
    UpdateWs u;
    uint32_t* bag;   // bag id of every occurrence slot (read for ragged tables only)
    char* partials;  // partial rows of pdim accumulator elements
    uint32_t* pany;  // per partial row: did any occurrence take part
    int64_t bytes;
};

inline AdaWs carve_adagrad_ws(char* base, int64_t n, int pdim) {
    AdaWs w;
    w.u = plan_index_ws(base, n);
    const int64_t max_partials = 2 * (n / kChunk) + 2;  // as the index phase counts them
    int64_t off = w.u.bytes;
    auto take = [&](int64_t bytes) -> char* {
        char* p = base ? base + off : nullptr;
        off += align256(bytes);
        return p;
    };
    w.bag = reinterpret_cast<uint32_t*>(take(4 * (n + 1)));
    w.partials = take(8 * max_partials * (int64_t)(pdim > 0 ? pdim : 4));
    w.pany = reinterpret_cast<uint32_t*>(take(4 * max_partials));
    w.bytes = off;
    return w;
}

inline bool ada_ragged(const et_adagrad_desc& d) { return d.colptr != nullptr; }
inline bool ada_work(const et_adagrad_desc& d) {
    return d.dim > 0 && d.batch > 0 && (ada_ragged(d) ? d.nnz > 0 : d.pool > 0);
}
inline int64_t ada_occurrences(const et_adagrad_desc& d) {
    return !ada_work(d) ? 0 : ada_ragged(d) ? d.nnz : (int64_t)d.pool * d.batch;
}

inline bool ranges_overlap(uintptr_t a, uint64_t na, uintptr_t b, uint64_t nb) {
    return a < b + nb && b < a + na;
}

// Descriptor checks (host only); *n_out = occurrences of all tables with work, *pdim_out the
// largest dim rounded up to a 16-byte row of floats.
inline int validate_adagrad(int dtype, const et_adagrad_desc* descs, int ntables, bool rowwise,
                            int64_t* n_out, int* pdim_out, bool need_ptrs) {
    if (ntables < 0) return fail(ET_ERR_ARG, "negative ntables");
    if (ntables > ET_MAX_TABLES_PER_LAUNCH)
        return fail(ET_ERR_ARG, "at most %d tables per update call", ET_MAX_TABLES_PER_LAUNCH);
    if (ntables > 0 && !descs) return fail(ET_ERR_ARG, "descs is NULL");
    const uint64_t es = (uint64_t)elsize(dtype), cs = dtype == ET_F64 ? 8u : 4u;
    int64_t n = 0;
    uint64_t rows = 0;
    int pdim = 0;
    for (int t = 0; t < ntables; ++t) {
        const et_adagrad_desc& d = descs[t];
        if (d.dim < 0 || d.pool < 0 || d.nrows < 0 || d.batch < 0 || d.cols_per_page < 0 ||
            d.nnz < 0)
            return fail(ET_ERR_ARG, "table %d: negative size", t);
        if (d.batch >= 0xffffffffll) return fail(ET_ERR_ARG, "table %d: batch too large", t);
        rows += (uint64_t)d.nrows;
        if (!ada_work(d)) continue;
        if (need_ptrs) {
            if (!d.idx || !d.table || !d.delta) return fail(ET_ERR_ARG, "table %d: NULL", t);
            if (!d.state) return fail(ET_ERR_ARG, "table %d: state is NULL", t);
        }
        if (!ada_ragged(d) && d.ld_idx < d.pool)
            return fail(ET_ERR_ARG, "table %d: ld_idx < pool", t);
        if (d.ld_table < d.dim || d.ld_delta < d.dim)
            return fail(ET_ERR_ARG, "table %d: leading dimension < dim", t);
        if (!rowwise && d.ld_state < d.dim)
            return fail(ET_ERR_ARG, "table %d: ld_state < dim", t);
        if (need_ptrs && d.nrows > 0) {
            const uint64_t sbytes =
                rowwise ? (uint64_t)d.nrows * cs
                        : ((uint64_t)(d.nrows - 1) * (uint64_t)d.ld_state + (uint64_t)d.dim) * cs;
            // a paged table is its array of page pointers here (the pages are device data)
            const uint64_t tbytes =
                d.cols_per_page > 0
                    ? (uint64_t)((d.nrows + d.cols_per_page - 1) / d.cols_per_page) * 8u
                    : ((uint64_t)(d.nrows - 1) * (uint64_t)d.ld_table + (uint64_t)d.dim) * es;
            if (ranges_overlap((uintptr_t)d.state, sbytes, (uintptr_t)d.table, tbytes))
                return fail(ET_ERR_ARG, "table %d: state overlaps the table", t);
        }
        n += ada_occurrences(d);
        if (n >= 0x7fffffffll) return fail(ET_ERR_ARG, "too many occurrences");
        if (d.dim > pdim) pdim = d.dim;
    }
    if (rows >= 0xffffffffull) return fail(ET_ERR_ARG, "too many table columns");
    *n_out = n;
    *pdim_out = (pdim + 3) & ~3;
    return ET_OK;
}

constexpr uint32_t kAdaFlags = ET_FLAG_NONTEMPORAL | ET_FLAG_ADAGRAD_ROWWISE;
constexpr uint32_t kAdaSgdOnly = ET_FLAG_F16_FP32_ACC | ET_FLAG_EXACT_UPDATE | ET_FLAG_SGD_UNFUSED |
                                 ET_FLAG_SGD_F64_ALPHA | ET_FLAG_SGD_INDEX_ONLY |
                                 ET_FLAG_SGD_APPLY_ONLY | ET_FLAG_SGD_HOT_PASS |
                                 ET_FLAG_EXACT_IF_FAST;

inline int check_adagrad_call(int dtype, uint32_t flags) {
    if (dtype != ET_F32 && dtype != ET_F64 && dtype != ET_F16 && dtype != ET_BF16)
        return fail(ET_ERR_UNSUPPORTED, "sparse AdaGrad: dtype %d", dtype);
    if (flags & kAdaSgdOnly)
        return fail(ET_ERR_UNSUPPORTED, "sparse AdaGrad: flags 0x%x belong to the SGD", flags & kAdaSgdOnly);
    if (flags & ~kAdaFlags) return fail(ET_ERR_ARG, "sparse AdaGrad: unknown flags 0x%x", flags & ~kAdaFlags);
    return ET_OK;
}

// f(Elem<T, C>{}, std::bool_constant<ROW>{}, std::bool_constant<NT>{})
template <typename F>
int dispatch_adagrad(int dtype, uint32_t flags, F&& f) {
    const bool nt = (flags & ET_FLAG_NONTEMPORAL) != 0;
    const bool row = (flags & ET_FLAG_ADAGRAD_ROWWISE) != 0;
    auto with_elem = [&](auto e) -> int {
        auto with_row = [&](auto r) -> int {
            return nt ? f(e, r, std::true_type{}) : f(e, r, std::false_type{});
        };
        return row ? with_row(std::true_type{}) : with_row(std::false_type{});
    };
    switch (dtype) {
        case ET_F32: return with_elem(Elem<float, float>{});
        case ET_F64: return with_elem(Elem<double, double>{});
        case ET_BF16: return with_elem(Elem<__bf16, float>{});
        default: return with_elem(Elem<_Float16, float>{});  // ET_F16
    }
}

struct AdaRun {
    UpdatePack pack;
    AdaPack ap;
    AdaWs w;
    Grouped gr;
    VecGroups vg;
    int ntables, pdim;
    int64_t n;
    uint32_t sent;
    bool any_generic;
    hipStream_t s;
};

template <typename T, typename C, bool ROW, bool NT>
int launch_adagrad(const AdaRun& r, C eta, C eps) {
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
                hipLaunchKernelGGL((k_adagrad_chunks<D, ROW, NT>), dim3(grid), dim3(256), 0, r.s,
                                   r.pack, r.ap, r.ntables, r.gr.vals, u.recs, u.counters, r.w.bag,
                                   partials, r.w.pany, r.pdim, r.sent, eta, eps, r.vg.mask[i]);
                hipLaunchKernelGGL((k_adagrad_combine<D, ROW, NT>),
                                   dim3((unsigned)(cb < 2048 ? cb : 2048)), dim3(256), 0, r.s,
                                   r.pack, r.ap, r.ntables, r.gr.keys, u.seg_start, u.multi,
                                   u.counters, u.mlist, partials, r.w.pany, r.pdim, r.sent, eta,
                                   eps, r.vg.mask[i]);
            });
        ET_LAUNCH_CHECK("k_adagrad_chunks");
    }
    if (r.any_generic) {
        C* partials = reinterpret_cast<C*>(r.w.partials);
        const int64_t cb = cdiv64(mmax, 4);
        hipLaunchKernelGGL((k_adagrad_chunks_generic<T, C, ROW, NT>), dim3(grid), dim3(256), 0, r.s,
                           r.pack, r.ap, r.ntables, r.gr.vals, u.recs, u.counters, r.w.bag,
                           partials, r.w.pany, r.pdim, r.sent, eta, eps);
        hipLaunchKernelGGL((k_adagrad_combine_generic<T, C, ROW, NT>),
                           dim3((unsigned)(cb < 4096 ? cb : 4096)), dim3(256), 0, r.s, r.pack, r.ap,
                           r.ntables, r.gr.keys, u.seg_start, u.multi, u.counters, u.mlist,
                           partials, r.w.pany, r.pdim, r.sent, eta, eps);
        ET_LAUNCH_CHECK("k_adagrad_chunks_generic");
    }
    return ET_OK;
}

// The front of the pipeline, shared with et_weighted_adagrad: descriptor checks, the workspace,
// the tables packed as vector or fixed-pool indices, the bag id of every ragged entry and
// group_occurrences.  run.n == 0 on return means there is nothing to launch.
inline int prepare_adagrad(int dtype, const et_adagrad_desc* descs, int ntables, bool rowwise,
                           void* workspace, int64_t ws_bytes, void* stream, AdaRun& run) {
    int rc = validate_adagrad(dtype, descs, ntables, rowwise, &run.n, &run.pdim, true);
    if (rc != ET_OK) return rc;
    if (run.n == 0) return ET_OK;
    run.w = carve_adagrad_ws(static_cast<char*>(workspace), run.n, run.pdim);
    if (!workspace || ws_bytes < run.w.bytes)
        return fail(ET_ERR_WORKSPACE, "workspace of %lld bytes needed", (long long)run.w.bytes);
    run.ntables = ntables;
    run.s = static_cast<hipStream_t>(stream);

    // fixed-pool tables as they are, ragged ones as a vector index over their values
    UpdatePack& pack = run.pack;
    RaggedBagArgs ba{};
    uint32_t ro = 0, oo = 0;
    int64_t max_batch = 0;
    pack.vec_mask = 0;
    run.ap.ragged = 0;
    run.any_generic = false;
    for (int t = 0; t < ntables; ++t) {
        const et_adagrad_desc& a = descs[t];
        const bool work = ada_work(a), ragged = ada_ragged(a);
        et_update_desc d{};
        d.table = a.table;
        d.ld_table = a.ld_table;
        d.nrows = a.nrows;
        d.dim = a.dim;
        d.pool = ragged ? 1 : a.pool;
        d.delta = a.delta;
        d.ld_delta = a.ld_delta;
        d.idx = a.idx;
        d.ld_idx = ragged ? 1 : a.ld_idx;
        d.batch = !work ? 0 : ragged ? a.nnz : a.batch;
        d.cols_per_page = a.cols_per_page;
        pack.d[t] = d;
        pack.row_off[t] = ro;
        pack.occ_off[t] = oo;
        run.ap.state[t] = a.state;
        run.ap.ld_state[t] = a.ld_state;
        ba.colptr[t] = a.colptr;
        ba.batch[t] = work && ragged ? a.batch : 0;
        ba.nnz[t] = work && ragged ? a.nnz : 0;
        ba.off[t] = (int64_t)oo;
        ro += (uint32_t)a.nrows;
        oo += (uint32_t)((int64_t)d.pool * d.batch);
        if (!work) continue;
        if (ragged) {
            run.ap.ragged |= 1u << t;
            if (a.batch > max_batch) max_batch = a.batch;
        }
        // the vector kernels: Float32 rows, gradient rows and state rows of 16-byte multiples
        const bool vec = dtype == ET_F32 && (a.cols_per_page > 0 || aligned16(a.table)) &&
                         a.ld_table % 4 == 0 && a.dim % 4 == 0 && a.dim <= 2048 &&
                         aligned16(a.delta) && a.ld_delta % 4 == 0 &&
                         (rowwise ? ((uintptr_t)a.state & 3u) == 0
                                  : aligned16(a.state) && a.ld_state % 4 == 0);
        if (vec && run.vg.add(vec_dim_ok(a.dim) ? a.dim : masked_capacity(a.dim), t))
            pack.vec_mask |= 1u << t;
        else
            run.any_generic = true;
    }
    pack.row_off[ntables] = ro;
    pack.occ_off[ntables] = oo;
    run.sent = ro;  // key of out-of-range indices (sorts last)

    if (run.ap.ragged) {
        ET_HIP_CHECK(hipMemsetAsync(run.w.bag, 0, (size_t)run.n * 4, run.s));
        rc = launch_ragged_bag_ids<uint32_t>(ba, ntables, max_batch, run.w.bag, run.s);
        if (rc != ET_OK) return rc;
    }
    return group_occurrences(pack, ntables, run.n, run.sent, kChunk, run.w.u, run.gr, run.s);
}

}  // namespace et

extern "C" int et_adagrad_workspace_size(const et_adagrad_desc* descs, int32_t ntables,
                                         int64_t* bytes) {
    et::clear_err();
    if (!bytes) return et::fail(ET_ERR_ARG, "bytes is NULL");
    int64_t n;
    int pdim;
    // sized for either form and any float type: only the sizes are read
    const int rc = et::validate_adagrad(ET_F32, descs, ntables, true, &n, &pdim, false);
    if (rc != ET_OK) return rc;
    *bytes = et::carve_adagrad_ws(nullptr, n, pdim).bytes;
    return ET_OK;
}

extern "C" int et_sparse_adagrad(int dtype, const et_adagrad_desc* descs, int32_t ntables,
                                 double eta, double eps, uint32_t flags, void* workspace,
                                 int64_t ws_bytes, void* stream) {
    et::clear_err();
    int rc = et::check_adagrad_call(dtype, flags);
    if (rc != ET_OK) return rc;
    et::AdaRun run;
    rc = et::prepare_adagrad(dtype, descs, ntables, (flags & ET_FLAG_ADAGRAD_ROWWISE) != 0,
                             workspace, ws_bytes, stream, run);
    if (rc != ET_OK || run.n == 0) return rc;
    return et::dispatch_adagrad(dtype, flags, [&](auto e, auto row, auto nt) {
        using T = typename decltype(e)::type;
        using C = typename decltype(e)::acc;
        return et::launch_adagrad<T, C, decltype(row)::value, decltype(nt)::value>(run, (C)eta,
                                                                                    (C)eps);
    });
}
