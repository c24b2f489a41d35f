// et_quant.hip — row-wise quantised tables (INT8 / INT4 rows with a Float16 scale and bias per
// row): the pooled lookup with the dequantisation fused into the sum, and the quantiser.
// Textually included at the end of et_lookup.hip: it reuses idx_row32, ragged_range, the store
// helpers, note_oob, the stripe placement (et_lookup_order.h) and the lookup tuning of that
// translation unit, and counts out-of-range indices in its counter.
//
// The format and the arithmetic are defined in include/embtab.h.  What matters here:
//   * v = float(q) * float(scale) + float(bias) has an exact product (8 x 11 significant bits),
//     so one fused multiply-add per feature gives the one rounding the contract asks for — the
//     Float32 result equals the float kernels' on the dequantised table bit for bit;
//   * a bag's sum is a COPY of its first row's v, then v of the other rows added one at a time
//     in index order, in Float32; the store converts once.
//
// Vector kernel.  A lane owns 16 payload bytes of a row — 16 features (INT8) or 32 (INT4), one
// Float32 accumulator each — so a row of `vpr` 16-byte vectors is a lane group of LPR lanes
// (the power-of-two capacity of vpr; lanes beyond the row re-read its last vector and never
// store): D = 128 is 8 lanes per bag for INT8 and 4 for INT4, 8 or 16 bags per wave.  Eight rows
// per group are issued before the first is consumed; each row is one 16-byte payload load and
// one 4-byte header load (every lane of the group reads the same dword) issued together.  A
// bag's indices are read once by the group's lanes (8 at least per round: lanes of narrow
// groups load several) and handed round with ds_bpermute, as et_ragged.hip does; fixed-pool and
// ragged bags differ only in where the bag's range comes from.  No LDS, no barriers.
//
// Schedule: the static XCD stripe schedule of k_pooled_vec_striped (workgroup b on XCD b % 8
// runs stripe entries placed by et_order::place_stripes, so an XCD's L2 holds few light
// tables).  Per-XCD queues, L2 order and CU affinity are not applied to this kernel.

namespace et {

struct QuantPack {
    et_quant_desc d[ET_MAX_TABLES_PER_LAUNCH];
};

// table (bits 0-4) | stripe (bits 5-7) of the entries each XCD owns
struct QuantStripes {
    uint8_t e[kXcds][ET_MAX_TABLES_PER_LAUNCH];
};
static_assert(ET_MAX_TABLES_PER_LAUNCH <= 32 && kXcds <= 8, "QuantStripes entry encoding");

__device__ __forceinline__ float half_bits_f32(uint32_t bits16) {
    const uint16_t u = (uint16_t)bits16;
    _Float16 h;
    __builtin_memcpy(&h, &u, 2);
    return (float)h;
}

// Bag `bag` of a table: its first index, its length and the number of ragged bounds that had
// to be clamped (0 for a fixed pool).
__device__ __forceinline__ void quant_bag(const et_quant_desc& d, int64_t bag,
                                          const int64_t*& ip, int64_t& len,
                                          int& clamped) {
    if (d.colptr) {
        int64_t lo, hi;
        ragged_range(d.colptr, bag, d.nnz, lo, hi, clamped);
        ip = d.idx + lo;
        len = hi - lo;
    } else {
        clamped = 0;
        ip = d.idx + bag * d.ld_idx;
        len = d.pool;
    }
}

template <int BITS, int LPR>
struct QuantGeom {
    static constexpr int F = 128 / BITS;            // features (accumulators) per lane
    static constexpr int GPW = 64 / LPR;            // bags per wave
    static constexpr int U = 8;                     // rows in flight per group
    static constexpr int CH = LPR > U ? LPR : U;    // indices per chunk of a bag
    static constexpr int K = CH / LPR;              // of which each lane loads K
};

// The 16 payload bytes of a lane as F unsigned values, in feature order.
template <int BITS>
__device__ __forceinline__ void quant_unpack(u32x4 p, float (&q)[128 / BITS]) {
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        if constexpr (BITS == 8) {
#pragma unroll
            for (int k = 0; k < 4; ++k) q[4 * w + k] = (float)((p[w] >> (8 * k)) & 0xffu);
        } else {
            uint32_t lo = p[w] & 0x0f0f0f0fu, hi = (p[w] >> 4) & 0x0f0f0f0fu;
            // opaque: keep the two words whole, so each nibble is one byte-to-float conversion
            // (otherwise the shifts are merged and every feature costs a shift, a mask and one)
            asm("" : "+v"(lo));
            asm("" : "+v"(hi));
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                q[8 * w + 2 * k] = (float)((lo >> (8 * k)) & 0xffu);
                q[8 * w + 2 * k + 1] = (float)((hi >> (8 * k)) & 0xffu);
            }
        }
    }
}

// Slot i of the group's current index chunk: lane (i % LPR) of the group loaded it as its
// myr[i / LPR].  With a compile-time i the select chain folds away.
template <int LPR, int K>
__device__ __forceinline__ uint32_t quant_slot(const uint32_t (&myr)[K], int gbase, int i) {
    uint32_t r = myr[0];
    if constexpr (K > 1) {
        const int m = i / LPR;
#pragma unroll
        for (int mm = 1; mm < K; ++mm) r = m == mm ? myr[mm] : r;
    }
    if constexpr (LPR == 1) return r;
    return (uint32_t)__shfl((int)r, gbase + i % LPR, 64);
}

// UU rows of one bag (slots i0 .. i0+UU-1, all valid): every payload and header load is issued
// before the first row is consumed, then the rows are added in slot order.  The accumulators
// start at -0.0, the identity of the Float32 add (-0 + v == v bit for bit, for v = -0 too), so
// the first row is a copy without a select.  An out-of-range
// index reads row 0 with a zero header, so it adds +0 to every feature.
//   hbase / hstride: the header of row r is the dword at hbase + r * hstride (fused:
//   table + payload, ld_bytes; split: hdr, 4)
template <int BITS, int LPR, int UU>
__device__ __forceinline__ void quant_load_add(
    const char* __restrict__ table, uint32_t ldb, const char* __restrict__ hbase, uint32_t hstride,
    const uint32_t (&myr)[QuantGeom<BITS, LPR>::K], int gbase, int i0, uint32_t voff,
    float (&acc)[QuantGeom<BITS, LPR>::F], int& bad) {
    using G = QuantGeom<BITS, LPR>;
    constexpr int F = G::F;
    u32x4 buf[UU];
    uint32_t hd[UU];
    bool ok[UU];
#pragma unroll
    for (int u = 0; u < UU; ++u) {
        const uint32_t r = quant_slot<LPR, G::K>(myr, gbase, i0 + u);
        ok[u] = r != ~0u;
        const uint32_t row = ok[u] ? r : 0u;
        buf[u] = *reinterpret_cast<const u32x4*>(table + (uint64_t)row * ldb + voff);
        hd[u] = *reinterpret_cast<const uint32_t*>(hbase + (uint64_t)row * hstride);
    }
#pragma unroll
    for (int u = 0; u < UU; ++u) {
        bad += ok[u] ? 0 : 1;
        const uint32_t h = ok[u] ? hd[u] : 0u;
        const float s = half_bits_f32(h & 0xffffu), b = half_bits_f32(h >> 16);
        float q[F];
        quant_unpack<BITS>(buf[u], q);
#pragma unroll
        for (int f = 0; f < F; ++f) {
            const float v = __builtin_fmaf(q[f], s, b);  // exact product: one rounding
            acc[f] = acc[f] + v;
        }
    }
}

__device__ __forceinline__ bool quant_aligned16(const void* p) {
    return (reinterpret_cast<uintptr_t>(p) & 15u) == 0;
}

// Store a lane's F converted values at p: 16-byte stores when `al` (p is 16-byte aligned: a
// lane's block is a multiple of 32 bytes), element stores otherwise.
template <typename O, int F>
__device__ __forceinline__ void quant_store(O* __restrict__ p, const float (&acc)[F], bool al,
                                            int nt) {
    constexpr int N = 16 / (int)sizeof(O);
    if (al) {
#pragma unroll
        for (int v = 0; v < F / N; ++v) {
            O y[N];
#pragma unroll
            for (int k = 0; k < N; ++k) y[k] = O(acc[v * N + k]);
            if (nt)
                store16<true>(reinterpret_cast<u32x4*>(p) + v, pack16<O, N>(y));
            else
                store16<false>(reinterpret_cast<u32x4*>(p) + v, pack16<O, N>(y));
        }
    } else {
#pragma unroll
        for (int f = 0; f < F; ++f) {
            if (nt)
                store_scalar<true>(p + f, O(acc[f]));
            else
                store_scalar<false>(p + f, O(acc[f]));
        }
    }
}

// Vector kernel: grid = kXcds * ntables * stripe_chunks workgroups of 256; a workgroup owns
// 4 * GPW consecutive bags of one table.  `out` is the destination's ET_* element type.
template <int BITS, int LPR>
__global__ __launch_bounds__(256) void k_quant_vec(QuantPack pack, QuantStripes sm, int ntables,
                                                   int64_t batch, void* __restrict__ dst,
                                                   int64_t ld_dst, int out, int nt,
                                                   int64_t stripe_chunks, int64_t nchunks) {
    using G = QuantGeom<BITS, LPR>;
    constexpr int F = G::F, CH = G::CH, K = G::K, U = G::U;
    const int x = blockIdx.x % kXcds;
    const int64_t slot = blockIdx.x / kXcds;
    const uint32_t e = sm.e[x][slot % ntables];
    const int64_t j = slot / ntables;
    const int64_t chunk = (int64_t)(e >> 5) * stripe_chunks + j;
    if (j >= stripe_chunks || chunk >= nchunks) return;
    const et_quant_desc& d = pack.d[e & 31u];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = lane / LPR, sub = lane % LPR, gbase = g * LPR;
    const int64_t bag = chunk * (4 * G::GPW) + wave * G::GPW + g;
    if (bag >= batch) return;

    const char* table = reinterpret_cast<const char*>(d.table);
    const uint32_t ldb = (uint32_t)d.ld_bytes, nr = (uint32_t)d.nrows;
    const uint32_t payload = (uint32_t)d.dim * BITS / 8u;
    const int vpr = (int)(payload / 16u);
    const char* hbase = d.hdr ? reinterpret_cast<const char*>(d.hdr) : table + payload;
    const uint32_t hstride = d.hdr ? 4u : ldb;
    const uint32_t voff = 16u * (uint32_t)(sub < vpr ? sub : vpr - 1);
    const int64_t* ip;
    int64_t len;
    int bad;
    quant_bag(d, bag, ip, len, bad);

    float acc[F];
#pragma unroll
    for (int f = 0; f < F; ++f) acc[f] = -0.f;

    for (int64_t c0 = 0; c0 < len; c0 += CH) {
        const int cnt = len - c0 < CH ? (int)(len - c0) : CH;
        uint32_t myr[K];  // lanes past the end re-read the chunk's last index
#pragma unroll
        for (int m = 0; m < K; ++m) {
            const int i = m * LPR + sub;
            myr[m] = idx_row32((long long)ip[c0 + (i < cnt ? i : cnt - 1)], nr);
        }
#define ET_Q_LOAD_ADD(UU, I0)                                                                  \
    quant_load_add<BITS, LPR, UU>(table, ldb, hbase, hstride, myr, gbase, I0, voff, acc, bad)
        int i0 = 0;
        if constexpr (K > 1) {
            // CH == U: a full chunk is one batch at compile-time slots
            if (cnt == CH) {
                ET_Q_LOAD_ADD(U, 0);
                i0 = CH;
            }
        } else {
            for (; i0 + U <= cnt; i0 += U) ET_Q_LOAD_ADD(U, i0);
        }
        if (cnt - i0 >= 4) {
            ET_Q_LOAD_ADD(4, i0);
            i0 += 4;
        }
        if (cnt - i0 >= 2) {
            ET_Q_LOAD_ADD(2, i0);
            i0 += 2;
        }
        if (cnt - i0 >= 1) ET_Q_LOAD_ADD(1, i0);
#undef ET_Q_LOAD_ADD
    }
    if (bad && sub == 0) note_oob(bad);
    if (sub >= vpr) return;
    if (len <= 0) {  // an empty bag is +0
#pragma unroll
        for (int f = 0; f < F; ++f) acc[f] = 0.f;
    }
    const int64_t o = bag * ld_dst + d.dst_row_off + (int64_t)sub * F;
    if (out == ET_F32) {
        float* p = reinterpret_cast<float*>(dst) + o;
        quant_store<float, F>(p, acc, quant_aligned16(p), nt);
    } else if (out == ET_F16) {
        _Float16* p = reinterpret_cast<_Float16*>(dst) + o;
        quant_store<_Float16, F>(p, acc, quant_aligned16(p), nt);
    } else {
        __bf16* p = reinterpret_cast<__bf16*>(dst) + o;
        quant_store<__bf16, F>(p, acc, quant_aligned16(p), nt);
    }
}

// Generic kernel: any dim, alignment and leading dimension (byte reads only).  One wave per bag,
// lanes stride over the features, the bag's rows sequential per feature.
template <typename O>
__global__ __launch_bounds__(256) void k_quant_generic(QuantPack pack, int ntables, int64_t batch,
                                                       O* __restrict__ dst, int64_t ld_dst,
                                                       int nt) {
    constexpr int K = 4;
    const int64_t item = blockIdx.x;
    const et_quant_desc& d = pack.d[(int)(item % ntables)];
    const int64_t chunk = item / ntables;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t bag = chunk * 4 + wave;
    if (bag >= batch) return;
    const int64_t* ip;
    int64_t len;
    int clamped;
    quant_bag(d, bag, ip, len, clamped);
    if (clamped && lane == 0) note_oob(clamped);
    const uint8_t* table = reinterpret_cast<const uint8_t*>(d.table);
    const uint8_t* hdr = reinterpret_cast<const uint8_t*>(d.hdr);
    const int dim = d.dim, bits = d.bits;
    const int64_t payload = (int64_t)dim * bits / 8;
    O* out = dst + bag * ld_dst + d.dst_row_off;
    for (int f0 = 0; f0 < dim; f0 += 64 * K) {
        float acc[K];
#pragma unroll
        for (int k = 0; k < K; ++k) acc[k] = 0.f;
        for (int64_t i = 0; i < len; ++i) {
            uint64_t row = (uint64_t)(ip[i] - 1);
            const bool ok = row < (uint64_t)d.nrows;
            if (!ok && lane == 0 && f0 == 0) note_oob();
            row = ok ? row : 0;
            const uint8_t* r = table + row * (uint64_t)d.ld_bytes;
            const uint8_t* h = hdr ? hdr + row * 4u : r + payload;
            const float s = ok ? half_bits_f32((uint32_t)h[0] | ((uint32_t)h[1] << 8)) : 0.f;
            const float b = ok ? half_bits_f32((uint32_t)h[2] | ((uint32_t)h[3] << 8)) : 0.f;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const int f = f0 + lane + 64 * k;
                if (f < dim) {
                    const uint32_t q =
                        bits == 8 ? (uint32_t)r[f] : ((uint32_t)r[f >> 1] >> ((f & 1) * 4)) & 15u;
                    const float v = __builtin_fmaf((float)q, s, b);
                    acc[k] = i == 0 ? v : acc[k] + v;
                }
            }
        }
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int f = f0 + lane + 64 * k;
            if (f < dim) {
                if (nt)
                    store_scalar<true>(out + f, O(acc[k]));
                else
                    store_scalar<false>(out + f, O(acc[k]));
            }
        }
    }
}

// Quantiser (not a hot path): one wave per row, include/embtab.h's arithmetic.  Byte stores
// only, so any alignment; writes the payload and the header, never the padding.
__global__ __launch_bounds__(256) void k_quantize_rows(const float* __restrict__ src,
                                                       int64_t ld_src, int64_t nrows, int dim,
                                                       int bits, uint8_t* __restrict__ table,
                                                       int64_t ld_bytes, uint8_t* __restrict__ hdr) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t row = (int64_t)blockIdx.x * 4 + wave;
    if (row >= nrows) return;
    const float* x = src + row * ld_src;
    float lo = __builtin_inff(), hi = -__builtin_inff();
    for (int f = lane; f < dim; f += 64) {
        lo = fminf(lo, x[f]);
        hi = fmaxf(hi, x[f]);
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, m, 64));
        hi = fmaxf(hi, __shfl_xor(hi, m, 64));
    }
    const float L = (float)((1 << bits) - 1);
    _Float16 bh = (_Float16)lo;
    const float b = (float)bh;
    _Float16 sh = (_Float16)((hi - b) / L);
    float s = (float)sh;
    if (!(s > 0.f && s < __builtin_inff())) {
        sh = (_Float16)1.0f;
        s = 1.0f;
    }
    auto quant = [&](int f) -> uint32_t {
        return (uint32_t)fminf(fmaxf(rintf((x[f] - b) / s), 0.f), L);
    };
    uint8_t* out = table + row * ld_bytes;
    if (bits == 8) {
        for (int f = lane; f < dim; f += 64) out[f] = (uint8_t)quant(f);
    } else {
        for (int k = lane; k < dim / 2; k += 64)
            out[k] = (uint8_t)(quant(2 * k) | (quant(2 * k + 1) << 4));
    }
    if (lane == 0) {
        uint16_t su, bu;
        __builtin_memcpy(&su, &sh, 2);
        __builtin_memcpy(&bu, &bh, 2);
        uint8_t* h = hdr ? hdr + row * 4 : out + (int64_t)dim * bits / 8;
        h[0] = (uint8_t)(su & 0xff);
        h[1] = (uint8_t)(su >> 8);
        h[2] = (uint8_t)(bu & 0xff);
        h[3] = (uint8_t)(bu >> 8);
    }
}

// ---------------------------------------------------------------------------
// Host dispatch
// ---------------------------------------------------------------------------

// ET_ERR_ARG unless (dim, bits, ld_bytes) describe a row of the format; *payload = its bytes.
inline int quant_row_check(const char* what, int t, int32_t dim, int32_t bits, int64_t ld_bytes,
                           bool fused, int64_t* payload) {
    if (bits != 8 && bits != 4) return fail(ET_ERR_ARG, "%s %d: bits %d is not 8 or 4", what, t, bits);
    if (dim < 0) return fail(ET_ERR_ARG, "%s %d: negative dim", what, t);
    if (bits == 4 && (dim & 1)) return fail(ET_ERR_ARG, "%s %d: odd dim %d with 4 bits", what, t, dim);
    *payload = (int64_t)dim * bits / 8;
    if (ld_bytes < 0 || ld_bytes % 4 != 0)
        return fail(ET_ERR_ARG, "%s %d: ld_bytes %lld is not a non-negative multiple of 4", what, t,
                    (long long)ld_bytes);
    if (ld_bytes < *payload + (fused ? 4 : 0))
        return fail(ET_ERR_ARG, "%s %d: ld_bytes %lld < %lld (payload%s)", what, t,
                    (long long)ld_bytes, (long long)(*payload + (fused ? 4 : 0)),
                    fused ? " + fused header" : "");
    return ET_OK;
}

// Lane-group capacity of a row of vpr 16-byte vectors, 0 if it has no vector kernel.
inline int quant_lpr(int64_t vpr) {
    if (vpr < 1 || vpr > 64) return 0;
    int c = 1;
    while (c < vpr) c <<= 1;
    return c;
}

template <int BITS, int LPR>
int launch_quant_vec(const QuantPack& pack, int n, int64_t batch, void* dst, int64_t ld_dst,
                     int out, bool nt, hipStream_t s) {
    const int64_t per = 4 * QuantGeom<BITS, LPR>::GPW;
    const int64_t nchunks = (batch + per - 1) / per;
    const int64_t stripe_chunks = (nchunks + kXcds - 1) / kXcds;
    const int64_t grid = (int64_t)kXcds * n * stripe_chunks;
    if (grid > 0x7fffffffll) return fail(ET_ERR_ARG, "grid too large");
    int64_t bytes[ET_MAX_TABLES_PER_LAUNCH];
    for (int t = 0; t < n; ++t) bytes[t] = pack.d[t].nrows * pack.d[t].ld_bytes;
    uint32_t entry[kXcds][et_order::kMaxEntries];
    int nheavy = 0;
    const int nent = et_order::place_stripes(bytes, n, tuning().light_bytes, entry, &nheavy);
    if (nent != n) return fail(ET_ERR_HIP, "stripe placement gave %d entries for %d tables", nent, n);
    QuantStripes sm;
    memset(&sm, 0, sizeof(sm));
    for (int x = 0; x < kXcds; ++x)
        for (int k = 0; k < n; ++k)
            sm.e[x][k] = (uint8_t)((entry[x][k] & 31u) | (((entry[x][k] >> 8) & 7u) << 5));
    hipLaunchKernelGGL((k_quant_vec<BITS, LPR>), dim3((unsigned)grid), dim3(256), 0, s, pack, sm, n,
                       batch, dst, ld_dst, out, nt ? 1 : 0, stripe_chunks, nchunks);
    ET_LAUNCH_CHECK("k_quant_vec");
    return ET_OK;
}

template <int BITS>
int launch_quant_vec_bits(int lpr, const QuantPack& pack, int n, int64_t batch, void* dst,
                          int64_t ld_dst, int out, bool nt, hipStream_t s) {
    switch (lpr) {
        case 1: return launch_quant_vec<BITS, 1>(pack, n, batch, dst, ld_dst, out, nt, s);
        case 2: return launch_quant_vec<BITS, 2>(pack, n, batch, dst, ld_dst, out, nt, s);
        case 4: return launch_quant_vec<BITS, 4>(pack, n, batch, dst, ld_dst, out, nt, s);
        case 8: return launch_quant_vec<BITS, 8>(pack, n, batch, dst, ld_dst, out, nt, s);
        case 16: return launch_quant_vec<BITS, 16>(pack, n, batch, dst, ld_dst, out, nt, s);
        case 32: return launch_quant_vec<BITS, 32>(pack, n, batch, dst, ld_dst, out, nt, s);
        case 64: return launch_quant_vec<BITS, 64>(pack, n, batch, dst, ld_dst, out, nt, s);
    }
    return fail(ET_ERR_UNSUPPORTED, "quantised vector lane group %d", lpr);
}

template <typename O>
int launch_quant_generic(const QuantPack& pack, int n, int64_t batch, void* dst, int64_t ld_dst,
                         bool nt, hipStream_t s) {
    const int64_t grid = (batch + 3) / 4 * n;
    if (grid > 0x7fffffffll) return fail(ET_ERR_ARG, "grid too large");
    hipLaunchKernelGGL((k_quant_generic<O>), dim3((unsigned)grid), dim3(256), 0, s, pack, n, batch,
                       reinterpret_cast<O*>(dst), ld_dst, nt ? 1 : 0);
    ET_LAUNCH_CHECK("k_quant_generic");
    return ET_OK;
}

// Validate (everything before any device work), group the tables by kernel and launch one
// kernel per group: key 0 = generic, else bits * 256 + lane-group capacity.
inline int quant_dispatch(int out, const et_quant_desc* descs, int ntables, int64_t batch,
                          void* dst, int64_t ld_dst, uint32_t flags, hipStream_t s) {
    if (out != ET_F32 && out != ET_F16 && out != ET_BF16)
        return fail(ET_ERR_UNSUPPORTED, "destination dtype %d (Float32, Float16 or BFloat16)", out);
    if (flags & ~ET_FLAG_NONTEMPORAL)
        return fail(ET_ERR_UNSUPPORTED, "flags 0x%x: a quantised lookup takes the non-temporal flag only", flags);
    if (ntables < 0 || batch < 0) return fail(ET_ERR_ARG, "negative ntables/batch");
    if (ntables > ET_MAX_TABLES_PER_LAUNCH)
        return fail(ET_ERR_ARG, "at most %d tables per quantised lookup", ET_MAX_TABLES_PER_LAUNCH);
    if (ntables == 0 || batch == 0) return ET_OK;
    if (batch >= 0x7fffffffll) return fail(ET_ERR_ARG, "batch too large");
    if (!descs) return fail(ET_ERR_ARG, "descs is NULL");
    if (!dst) return fail(ET_ERR_ARG, "dst is NULL");
    int key_of[ET_MAX_TABLES_PER_LAUNCH];  // -1 nothing to do
    for (int t = 0; t < ntables; ++t) {
        const et_quant_desc& d = descs[t];
        int64_t payload = 0;
        const int rc = quant_row_check("table", t, d.dim, d.bits, d.ld_bytes, d.hdr == nullptr,
                                       &payload);
        if (rc != ET_OK) return rc;
        const bool ragged = d.colptr != nullptr;
        if (d.nrows < 0 || (ragged ? d.nnz < 0 : d.pool < 0 || d.ld_idx < 0))
            return fail(ET_ERR_ARG, "table %d: negative nrows/pool/ld_idx/nnz", t);
        if (d.dim == 0) {
            key_of[t] = -1;
            continue;
        }
        if (d.dst_row_off < 0 || d.dst_row_off + d.dim > ld_dst)
            return fail(ET_ERR_ARG, "table %d: rows [%lld, %lld) outside ld_dst %lld", t,
                        (long long)d.dst_row_off, (long long)(d.dst_row_off + d.dim),
                        (long long)ld_dst);
        if (ragged ? d.nnz > 0 : d.pool > 0) {
            if (!d.table || !d.idx) return fail(ET_ERR_ARG, "table %d: NULL table/idx", t);
            if (d.nrows == 0) return fail(ET_ERR_ARG, "table %d: indices into an empty table", t);
            if (!ragged && d.ld_idx < d.pool) return fail(ET_ERR_ARG, "table %d: ld_idx < pool", t);
        }
        const int lpr = quant_lpr(payload / 16);
        const bool vec = lpr != 0 && payload % 16 == 0 && d.ld_bytes % 16 == 0 &&
                         aligned16(d.table) && (reinterpret_cast<uintptr_t>(d.hdr) & 3u) == 0 &&
                         d.nrows > 0 && d.nrows < 0xffffffffll && d.ld_bytes < 0xffffffffll;
        key_of[t] = vec ? d.bits * 256 + lpr : 0;
    }
    open_side_streams(s);
    const bool nt = (flags & ET_FLAG_NONTEMPORAL) != 0;
    bool done[ET_MAX_TABLES_PER_LAUNCH] = {false};
    for (int t0 = 0; t0 < ntables; ++t0) {
        if (done[t0] || key_of[t0] < 0) continue;
        QuantPack pack;
        int n = 0;
        for (int t = t0; t < ntables; ++t) {
            if (done[t] || key_of[t] != key_of[t0]) continue;
            pack.d[n++] = descs[t];
            done[t] = true;
        }
        const int key = key_of[t0];
        int rc;
        if (key == 0) {
            rc = out == ET_F32   ? launch_quant_generic<float>(pack, n, batch, dst, ld_dst, nt, s)
                 : out == ET_F16 ? launch_quant_generic<_Float16>(pack, n, batch, dst, ld_dst, nt, s)
                                 : launch_quant_generic<__bf16>(pack, n, batch, dst, ld_dst, nt, s);
        } else if (key / 256 == 8) {
            rc = launch_quant_vec_bits<8>(key % 256, pack, n, batch, dst, ld_dst, out, nt, s);
        } else {
            rc = launch_quant_vec_bits<4>(key % 256, pack, n, batch, dst, ld_dst, out, nt, s);
        }
        if (rc != ET_OK) return rc;
    }
    return ET_OK;
}

}  // namespace et

extern "C" int et_quantize_rows(const float* src, int64_t ld_src, int64_t nrows, int32_t dim,
                                int32_t bits, void* table, int64_t ld_bytes, void* hdr,
                                void* stream) {
    et::clear_err();
    int64_t payload = 0;
    const int rc = et::quant_row_check("quantise", 0, dim, bits, ld_bytes, hdr == nullptr, &payload);
    if (rc != ET_OK) return rc;
    if (nrows < 0) return et::fail(ET_ERR_ARG, "negative nrows");
    if (ld_src < dim) return et::fail(ET_ERR_ARG, "ld_src < dim");
    if (nrows == 0 || dim == 0) return ET_OK;
    if (!src || !table) return et::fail(ET_ERR_ARG, "NULL src/table");
    const int64_t grid = (nrows + 3) / 4;
    if (grid > 0x7fffffffll) return et::fail(ET_ERR_ARG, "grid too large");
    hipStream_t s = static_cast<hipStream_t>(stream);
    et::open_side_streams(s);
    hipLaunchKernelGGL(et::k_quantize_rows, dim3((unsigned)grid), dim3(256), 0, s, src, ld_src,
                       nrows, (int)dim, (int)bits, static_cast<uint8_t*>(table), ld_bytes,
                       static_cast<uint8_t*>(hdr));
    ET_LAUNCH_CHECK("k_quantize_rows");
    return ET_OK;
}

extern "C" int et_quant_maplookup_prealloc(int dst_dtype, const et_quant_desc* descs,
                                           int32_t ntables, int64_t batch, void* dst,
                                           int64_t ld_dst, uint32_t flags, void* stream) {
    et::clear_err();
    return et::quant_dispatch(dst_dtype, descs, ntables, batch, dst, ld_dst, flags,
                              static_cast<hipStream_t>(stream));
}
