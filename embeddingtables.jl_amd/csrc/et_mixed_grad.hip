// et_mixed_grad.hip — Float32 tables updated straight from Float16 / BFloat16 gradients
// (ET_FLAG_DELTA_F16 / ET_FLAG_DELTA_BF16 of et_sparse_adagrad and et_sparse_adam), textually
// included by et_update.hip after et_adam.hip.  The front of the pipeline never touches delta
// and is AdaGrad's unchanged; the combine pass reads Float32 partial rows only and is the
// existing one, unchanged.  New here is the chunk pass: the gather of 16-bit gradient rows,
// their sum in Float32 and, for single-chunk columns, the update in place.
//
// Semantics (include/embtab.h): p_c = p_c + C(delta[:, bag]) with C(.) the exact conversion of
// a 16-bit value to Float32; everything after the gradient sum g is the optimiser's definition
// word for word, so the results equal the unflagged call on delta converted to Float32.
//
// Lane layout.  The Float32 kernels give a chunk record D/4 lanes of 4 floats; a 16-bit
// gradient row would then be read 8 bytes per lane.  Here a record has D/8 lanes (capacity D
// = the power of two at or above dim, 8 .. 1024, masked below it; at most a wave) and every
// lane owns 8 consecutive features:
//   gradient    one 16-byte load per row and lane (8 values), eight loads per lane in flight,
//               converted in registers at the add: BFloat16 by a shift and a mask, Float16 by
//               v_cvt_f32_f16 on either half (denormals kept)
//   table row, AdaGrad state, Adam moments    two adjacent 16-byte vectors per lane
//   partial row of a multi-chunk column       the same two vectors, Float32, in the existing
//               `partials` layout (plain rows of pdim floats)
// Half the lanes per record is twice the records per wave.  The row-wise sum of squares is
// reduced inside the lane group with lane shuffles (no LDS, no barrier).
//
// Tables whose dim is no multiple of 8, or whose gradient is not 16-byte aligned with
// ld_delta a multiple of 8 elements, take k_adagrad_chunks_generic / k_adam_chunks_generic
// with the gradient element type as their last template argument.

namespace et {

template <int D>
struct Mix {
    static constexpr int VPR = D / 8;                // 8-feature units of a row of capacity D
    static constexpr int LPR = VPR < 64 ? VPR : 64;  // lanes per chunk record
    static constexpr int NV = VPR / LPR;             // units per lane
    static constexpr int GPW = 64 / LPR;             // records per wave
    static constexpr int U = NV >= 8 ? 1 : 8 / NV;   // gradient rows in flight per lane
};

typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));

// C(.) of the eight 16-bit values of one 16-byte vector, in feature order.
template <bool BF>
__device__ __forceinline__ void mix_cvt8(const u32x4& p, float (&f)[8]) {
    const uint32_t w[4] = {p.x, p.y, p.z, p.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        if constexpr (BF) {
            f[2 * e] = __uint_as_float(w[e] << 16);
            f[2 * e + 1] = __uint_as_float(w[e] & 0xffff0000u);
        } else {
            const f16x2 h = __builtin_bit_cast(f16x2, w[e]);
            f[2 * e] = (float)h.x;
            f[2 * e + 1] = (float)h.y;
        }
    }
}

__device__ __forceinline__ void mix_unpack(const u32x4 (&a)[2], float (&f)[8]) {
    f[0] = __uint_as_float(a[0].x), f[1] = __uint_as_float(a[0].y);
    f[2] = __uint_as_float(a[0].z), f[3] = __uint_as_float(a[0].w);
    f[4] = __uint_as_float(a[1].x), f[5] = __uint_as_float(a[1].y);
    f[6] = __uint_as_float(a[1].z), f[7] = __uint_as_float(a[1].w);
}

// The two 16-byte vectors of 8-feature unit i of a Float32 row.
__device__ __forceinline__ void mix_load(const float* __restrict__ row, int i, u32x4 (&a)[2]) {
    const u32x4* p = reinterpret_cast<const u32x4*>(row) + 2 * i;
    a[0] = p[0];
    a[1] = p[1];
}

template <bool NT>
__device__ __forceinline__ void mix_store(float* __restrict__ row, int i, const float (&f)[8]) {
    u32x4* p = reinterpret_cast<u32x4*>(row) + 2 * i;
    store16<NT>(p, u32x4{__float_as_uint(f[0]), __float_as_uint(f[1]), __float_as_uint(f[2]),
                         __float_as_uint(f[3])});
    store16<NT>(p + 1, u32x4{__float_as_uint(f[4]), __float_as_uint(f[5]), __float_as_uint(f[6]),
                             __float_as_uint(f[7])});
}

// acc += C(delta[:, bag]) over sorted occurrences [s0, s1) in order (one lane group): ada_occ_sum
// over 16-bit rows.  vix[v] is the lane's 8-feature unit of slice v (clamped into the row, so no
// byte beyond dim * 2 is read).  Control flow is uniform inside a lane group, not inside a wave.
template <int D, bool BF>
__device__ __forceinline__ bool mix_occ_sum(const uint16_t* __restrict__ delta, uint64_t ldd,
                                            uint32_t occ_off, uint32_t pool, bool ragged,
                                            const uint32_t* __restrict__ bag_ids,
                                            const uint32_t* __restrict__ vals, uint32_t s0,
                                            uint32_t s1, int g, int sub,
                                            const int (&vix)[Mix<D>::NV],
                                            float (&acc)[Mix<D>::NV][8]) {
    constexpr int LPR = Mix<D>::LPR, NV = Mix<D>::NV, U = Mix<D>::U;
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
                    float f[8];
                    mix_cvt8<BF>(buf[u][v], f);
#pragma unroll
                    for (int e = 0; e < 8; ++e) acc[v][e] = acc[v][e] + f[e];
                }
            }
        }
    }
    return any;
}

// (sum_f g_f^2) of one column, every lane of the group active; lanes past the row add nothing.
template <int D>
__device__ __forceinline__ float mix_sum_squares(const float (&g)[Mix<D>::NV][8], int sub,
                                                 int vpr) {
    constexpr int LPR = Mix<D>::LPR, NV = Mix<D>::NV;
    float ss = 0.0f;
#pragma unroll
    for (int v = 0; v < NV; ++v)
        if (sub + v * LPR < vpr) {
#pragma unroll
            for (int e = 0; e < 8; ++e) ss = ss + g[v][e] * g[v][e];
        }
#pragma unroll
    for (int m = LPR / 2; m >= 1; m >>= 1) ss = ss + __shfl_xor(ss, m, 64);
    return ss;
}

// A chunk of a multi-chunk column: its partial row in Float32, for the combine pass.
template <int D>
__device__ __forceinline__ void mix_store_partial(float* __restrict__ prow,
                                                  const float (&acc)[Mix<D>::NV][8], int sub,
                                                  int vpr) {
    constexpr int LPR = Mix<D>::LPR, NV = Mix<D>::NV;
#pragma unroll
    for (int v = 0; v < NV; ++v)
        if (sub + v * LPR < vpr) mix_store<false>(prow, sub + v * LPR, acc[v]);
}

// AdaGrad ----------------------------------------------------------------------------------

template <int D, bool BF, bool ROW, bool NT>
__global__ __launch_bounds__(256) void k_adagrad_chunks_mixed(
    UpdatePack pack, AdaPack ap, int ntables, const uint32_t* __restrict__ vals,
    const ChunkRec* __restrict__ recs, const uint32_t* __restrict__ counters,
    const uint32_t* __restrict__ bag_ids, float* __restrict__ partials,
    uint32_t* __restrict__ pany, int pdim, uint32_t sent, float eta, float eps,
    uint32_t my_mask) {
    constexpr int LPR = Mix<D>::LPR, NV = Mix<D>::NV, GPW = Mix<D>::GPW;
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
        const int vpr = d.dim / 8;
        int vix[NV];
        vec_index<LPR, NV>(sub, vpr, vix);
        const bool apply = r.dst == kApply;
        u32x4 x[NV][2], st[NV][2];
        float srow = 0.0f;
#pragma unroll
        for (int v = 0; v < NV; ++v)
            x[v][0] = x[v][1] = st[v][0] = st[v][1] = u32x4{0u, 0u, 0u, 0u};
        if (apply) {  // the column and its state first: their latency hides under the gathers
#pragma unroll
            for (int v = 0; v < NV; ++v) mix_load(w, vix[v], x[v]);
            if constexpr (ROW) {
                srow = *sp;
            } else {
#pragma unroll
                for (int v = 0; v < NV; ++v) mix_load(sp, vix[v], st[v]);
            }
        }
        float acc[NV][8];
#pragma unroll
        for (int v = 0; v < NV; ++v)
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[v][e] = 0.0f;
        const bool any = mix_occ_sum<D, BF>(reinterpret_cast<const uint16_t*>(d.delta),
                                            (uint64_t)d.ld_delta, pack.occ_off[t],
                                            (uint32_t)d.pool, (ap.ragged >> t) & 1u, bag_ids, vals,
                                            r.s0, r.s1, g, sub, vix, acc);
        if (!apply) {
            mix_store_partial<D>(partials + (uint64_t)r.dst * pdim, acc, sub, vpr);
            if (sub == 0) pany[r.dst] = any ? 1u : 0u;
            continue;
        }
        if (!any) continue;  // no participating entry: neither the column nor its state is written
        float dd = 0.0f;
        if constexpr (ROW) {
            const float s2 = srow + mix_sum_squares<D>(acc, sub, vpr) / (float)d.dim;
            dd = ada_sqrt(s2) + eps;
            if (sub == 0) store_scalar<NT>(sp, s2);
        }
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            float wi[8], si[8], wo[8], so[8];
            mix_unpack(x[v], wi);
            if constexpr (!ROW) mix_unpack(st[v], si);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                float de = dd;
                if constexpr (!ROW) {
                    so[e] = si[e] + acc[v][e] * acc[v][e];
                    de = ada_sqrt(so[e]) + eps;
                }
                wo[e] = ada_step<float, float>(wi[e], acc[v][e], de, eta);
            }
            if (sub + v * LPR < vpr) {
                if constexpr (!ROW) mix_store<NT>(sp, sub + v * LPR, so);
                mix_store<NT>(w, sub + v * LPR, wo);
            }
        }
    }
}

// Adam -------------------------------------------------------------------------------------

template <int D, bool BF, bool ROW, bool NT>
__global__ ET_ADAM_KERNEL __launch_bounds__(256) void k_adam_chunks_mixed(
    UpdatePack pack, AdamPack ap, int ntables, const uint32_t* __restrict__ vals,
    const ChunkRec* __restrict__ recs, const uint32_t* __restrict__ counters,
    const uint32_t* __restrict__ bag_ids, float* __restrict__ partials,
    uint32_t* __restrict__ pany, int pdim, uint32_t sent, AdamHyper<float> h, uint32_t my_mask) {
    constexpr int LPR = Mix<D>::LPR, NV = Mix<D>::NV, GPW = Mix<D>::GPW;
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
        const int vpr = d.dim / 8;
        int vix[NV];
        vec_index<LPR, NV>(sub, vpr, vix);
        const bool apply = r.dst == kApply;
        u32x4 x[NV][2], mo[NV][2], vo[NV][2];
        float vrow = 0.0f, c1 = 1.0f, c2 = 1.0f;
#pragma unroll
        for (int v = 0; v < NV; ++v)
            x[v][0] = x[v][1] = mo[v][0] = mo[v][1] = vo[v][0] = vo[v][1] = u32x4{0u, 0u, 0u, 0u};
        if (apply) {  // three row streams first: their latency hides under the gathers
#pragma unroll
            for (int v = 0; v < NV; ++v) mix_load(w, vix[v], x[v]);
#pragma unroll
            for (int v = 0; v < NV; ++v) mix_load(mp, vix[v], mo[v]);
            if constexpr (ROW) {
                vrow = *vp;
            } else {
#pragma unroll
                for (int v = 0; v < NV; ++v) mix_load(vp, vix[v], vo[v]);
            }
            const float* st = reinterpret_cast<const float*>(ap.step[t]);
            c1 = 1.0f - st[0];
            c2 = 1.0f - st[1];
        }
        float acc[NV][8];
#pragma unroll
        for (int v = 0; v < NV; ++v)
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[v][e] = 0.0f;
        const bool any = mix_occ_sum<D, BF>(reinterpret_cast<const uint16_t*>(d.delta),
                                            (uint64_t)d.ld_delta, pack.occ_off[t],
                                            (uint32_t)d.pool, (ap.ragged >> t) & 1u, bag_ids, vals,
                                            r.s0, r.s1, g, sub, vix, acc);
        if (!apply) {
            mix_store_partial<D>(partials + (uint64_t)r.dst * pdim, acc, sub, vpr);
            if (sub == 0) pany[r.dst] = any ? 1u : 0u;
            continue;
        }
        if (!any) continue;  // no participating entry: neither the column nor its moments
        float dd = 0.0f;
        if constexpr (ROW) {
            const float v2 = adam_v(vrow, mix_sum_squares<D>(acc, sub, vpr) / (float)d.dim, h);
            dd = adam_den(v2, c2, h.eps);
            if (sub == 0) store_scalar<NT>(vp, v2);
        }
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            float wi[8], mi[8], vi[8], wo[8], m2[8], v2[8];
            mix_unpack(x[v], wi);
            mix_unpack(mo[v], mi);
            if constexpr (!ROW) mix_unpack(vo[v], vi);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                m2[e] = adam_m(mi[e], acc[v][e], h);
                float de = dd;
                if constexpr (!ROW) {
                    v2[e] = adam_v(vi[e], acc[v][e] * acc[v][e], h);
                    de = adam_den(v2[e], c2, h.eps);
                }
                wo[e] = adam_step<float, float>(wi[e], m2[e], c1, de, h.eta);
            }
            if (sub + v * LPR < vpr) {
                mix_store<NT>(mp, sub + v * LPR, m2);
                if constexpr (!ROW) mix_store<NT>(vp, sub + v * LPR, v2);
                mix_store<NT>(w, sub + v * LPR, wo);
            }
        }
    }
}

// Host --------------------------------------------------------------------------------------

template <typename F>
void with_mixed_capacity(int cap, F&& f) {
    static_assert(ET_ADAM_VEC_MAX_DIM == 1024, "the capacities of the mixed vector kernels");
    with_capacity_in<8, 16, 32, 64, 128, 256, 512, 1024>(cap, f);
}

// f(std::bool_constant<BF>{}, std::bool_constant<ROW>{}, std::bool_constant<NT>{})
template <typename F>
int dispatch_mixed(uint32_t flags, F&& f) {
    const bool nt = (flags & ET_FLAG_NONTEMPORAL) != 0;
    const bool row = (flags & ET_FLAG_ADAGRAD_ROWWISE) != 0;
    auto with_bf = [&](auto bf) -> int {
        auto with_row = [&](auto r) -> int {
            return nt ? f(bf, r, std::true_type{}) : f(bf, r, std::false_type{});
        };
        return row ? with_row(std::true_type{}) : with_row(std::false_type{});
    };
    return (flags & ET_FLAG_DELTA_BF16) ? with_bf(std::true_type{}) : with_bf(std::false_type{});
}

// r.vg8 groups the vector tables by the capacity of the chunk pass (8 features a lane), r.vg
// by the capacity of the unchanged combine pass (4 floats a lane); pack.vec_mask is their
// union and every other table is the generic kernels'.
inline int launch_adagrad_mixed(const AdaRun& r, uint32_t flags, float eta, float eps) {
    return dispatch_mixed(flags, [&](auto bf, auto row, auto nt) -> int {
        constexpr bool BF = decltype(bf)::value, ROW = decltype(row)::value,
                       NT = decltype(nt)::value;
        using G = std::conditional_t<BF, __bf16, _Float16>;
        const unsigned grid = sgd_grid(r.n);
        const int64_t mmax = r.n / kChunk + 2;  // multi-chunk columns at most
        const UpdateWs& u = r.w.u;
        float* partials = reinterpret_cast<float*>(r.w.partials);
        for (int i = 0; i < r.vg8.n; ++i)
            with_mixed_capacity(r.vg8.cap[i], [&](auto cap) {
                constexpr int D = decltype(cap)::value;
                hipLaunchKernelGGL((k_adagrad_chunks_mixed<D, BF, ROW, NT>), dim3(grid), dim3(256),
                                   0, r.s, r.pack, r.ap, r.ntables, r.gr.vals, u.recs, u.counters,
                                   r.w.bag, partials, r.w.pany, r.pdim, r.sent, eta, eps,
                                   r.vg8.mask[i]);
            });
        for (int i = 0; i < r.vg.n; ++i)
            with_capacity(r.vg.cap[i], [&](auto cap) {
                constexpr int D = decltype(cap)::value;
                constexpr int GPW = D / 4 < 64 ? 64 / (D / 4) : 1;
                const int64_t cb = cdiv64(mmax, 4 * GPW);
                hipLaunchKernelGGL((k_adagrad_combine<D, ROW, NT>),
                                   dim3((unsigned)(cb < 2048 ? cb : 2048)), dim3(256), 0, r.s,
                                   r.pack, r.ap, r.ntables, r.gr.keys, u.seg_start, u.multi,
                                   u.counters, u.mlist, partials, r.w.pany, r.pdim, r.sent, eta,
                                   eps, r.vg.mask[i]);
            });
        ET_LAUNCH_CHECK("k_adagrad_chunks_mixed");
        if (r.any_generic) {
            const int64_t cb = cdiv64(mmax, 4);
            hipLaunchKernelGGL((k_adagrad_chunks_generic<float, float, ROW, NT, G>), dim3(grid),
                               dim3(256), 0, r.s, r.pack, r.ap, r.ntables, r.gr.vals, u.recs,
                               u.counters, r.w.bag, partials, r.w.pany, r.pdim, r.sent, eta, eps);
            hipLaunchKernelGGL((k_adagrad_combine_generic<float, float, ROW, NT>),
                               dim3((unsigned)(cb < 4096 ? cb : 4096)), dim3(256), 0, r.s, r.pack,
                               r.ap, r.ntables, r.gr.keys, u.seg_start, u.multi, u.counters,
                               u.mlist, partials, r.w.pany, r.pdim, r.sent, eta, eps);
            ET_LAUNCH_CHECK("k_adagrad_chunks_generic");
        }
        return ET_OK;
    });
}

inline int launch_adam_mixed(const AdaRun& r, const UpdatePack& mpack, const AdamPack& ap,
                             const AdamHyper<float>& h, uint32_t flags) {
    return dispatch_mixed(flags, [&](auto bf, auto row, auto nt) -> int {
        constexpr bool BF = decltype(bf)::value, ROW = decltype(row)::value,
                       NT = decltype(nt)::value;
        using G = std::conditional_t<BF, __bf16, _Float16>;
        hipLaunchKernelGGL((k_adam_advance<float>), dim3(1), dim3(64), 0, r.s, ap, r.ntables, h.b1,
                           h.b2);
        ET_LAUNCH_CHECK("k_adam_advance");
        const unsigned grid = sgd_grid(r.n);
        const int64_t mmax = r.n / kChunk + 2;  // multi-chunk columns at most
        const UpdateWs& u = r.w.u;
        float* partials = reinterpret_cast<float*>(r.w.partials);
        for (int i = 0; i < r.vg8.n; ++i)
            with_mixed_capacity(r.vg8.cap[i], [&](auto cap) {
                constexpr int D = decltype(cap)::value;
                hipLaunchKernelGGL((k_adam_chunks_mixed<D, BF, ROW, NT>), dim3(grid), dim3(256), 0,
                                   r.s, mpack, ap, r.ntables, r.gr.vals, u.recs, u.counters,
                                   r.w.bag, partials, r.w.pany, r.pdim, r.sent, h, r.vg8.mask[i]);
            });
        for (int i = 0; i < r.vg.n; ++i)
            with_adam_capacity(r.vg.cap[i], [&](auto cap) {
                constexpr int D = decltype(cap)::value;
                constexpr int GPW = D / 4 < 64 ? 64 / (D / 4) : 1;
                const int64_t cb = cdiv64(mmax, 4 * GPW);
                hipLaunchKernelGGL((k_adam_combine<D, ROW, NT>),
                                   dim3((unsigned)(cb < 2048 ? cb : 2048)), dim3(256), 0, r.s,
                                   mpack, ap, r.ntables, r.gr.keys, u.seg_start, u.multi,
                                   u.counters, u.mlist, partials, r.w.pany, r.pdim, r.sent, h,
                                   r.vg.mask[i]);
            });
        ET_LAUNCH_CHECK("k_adam_chunks_mixed");
        if (r.any_generic) {
            const int64_t cb = cdiv64(mmax, 4);
            hipLaunchKernelGGL((k_adam_chunks_generic<float, float, ROW, NT, G>), dim3(grid),
                               dim3(256), 0, r.s, mpack, ap, r.ntables, r.gr.vals, u.recs,
                               u.counters, r.w.bag, partials, r.w.pany, r.pdim, r.sent, h);
            hipLaunchKernelGGL((k_adam_combine_generic<float, float, ROW, NT>),
                               dim3((unsigned)(cb < 4096 ? cb : 4096)), dim3(256), 0, r.s, mpack,
                               ap, r.ntables, r.gr.keys, u.seg_start, u.multi, u.counters, u.mlist,
                               partials, r.w.pany, r.pdim, r.sent, h);
            ET_LAUNCH_CHECK("k_adam_chunks_generic");
        }
        return ET_OK;
    });
}

}  // namespace et
