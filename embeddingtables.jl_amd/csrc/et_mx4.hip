// et_mx4.hip — MXFP4 rows (OCP Microscaling FP4: 32 E2M1 codes under one shared E8M0 scale
// byte, no header and no bias): the pooled lookup with the dequantisation fused into the sum,
// and the quantiser.  Textually included behind et_fp8.hip: the descriptors, the bag and index
// plumbing (quant_bag, quant_slot, QuantGeom<4, LPR>, quant_store), the stripe schedule and the
// host validation are et_quant.hip's; only the trailer (dim / 32 scale bytes instead of a
// 4-byte header), the decode and the quantiser differ.  The format and the arithmetic are
// defined in include/embtab.h ("MXFP4 rows").
//
//   * v = E2M1(q) * 2^(e - 127) has no rounding at all, so a bag's Float32 sum is the float
//     kernels' on the dequantised table bit for bit.
//   * Decode is the hardware's: v_cvt_scalef32_pk_f32_fp4 turns the two nibbles of one byte of a
//     payload word (the byte picked by op_sel, no shift and no mask) into two Float32 values
//     already multiplied by the scale.  Its scale operand is a Float32 of which only the
//     exponent field is read, so the scale byte e goes in as e << 23.  Measured on every code
//     under every scale byte: low nibble first, e = 0 is 2^-127 with subnormal
//     results kept, e = 254 overflows to Inf, e = 255 gives NaN for every code — the contract
//     with nothing to patch.
//   * A lane of the vector kernel owns 16 payload bytes: 32 features, exactly one MX block and
//     one scale byte.  Per row it issues one 16-byte payload load and one byte load of its own
//     scale (a dword shared by four lanes would save no load instruction, cost a byte extract
//     per row and ask the split array for 4-byte alignment); the arithmetic is 16 conversions
//     and 32 adds — no fma, no header conversion.
//   * An out-of-range index must add +0 whatever row 1 holds, and a NaN scale byte makes NaN of
//     a zero code: the lane replaces the payload AND the scale byte of such a row by zeros
//     (code 0 under scale byte 0 is +0).
//   * Like the FP8 kernels these opt out of packed Float32 arithmetic: the adds are issued one
//     feature at a time (v_add_f32), every result is pinned bit for bit.

namespace et {

// Byte SEL of `w` as two Float32 values (low nibble, high nibble), times 2^(e - 127) for the
// scale operand s = bits(e << 23).
#define ET_MX4_CVT(w, s, SEL) __builtin_amdgcn_cvt_scalef32_pk_f32_fp4((w), (s), (SEL))

__device__ __forceinline__ float mx4_scale_operand(uint32_t e) {
    return __builtin_bit_cast(float, e << 23);
}

// Scale bytes of a row: dim / 32 of them, fused behind the payload or `mx4_hdr_stride` apart in
// the split array.
__host__ __device__ __forceinline__ uint32_t mx4_hdr_stride(uint32_t dim) {
    return (dim / 32u + 3u) & ~3u;
}

// quant_load_add for MXFP4 rows: UU rows of one bag (slots i0 .. i0+UU-1, all valid), every
// load issued before the first row is consumed, the rows added in slot order onto accumulators
// that start at -0.0.  An out-of-range slot loads row 0 and is then replaced by a zero payload
// under a zero scale byte.
//   sbase / sstride: the lane's scale byte of row r is at sbase + r * sstride
template <int LPR, int UU>
__device__ __forceinline__ void mx4_load_add(
    const char* __restrict__ table, uint32_t ldb, const uint8_t* __restrict__ sbase,
    uint32_t sstride, const uint32_t (&myr)[QuantGeom<4, LPR>::K], int gbase, int i0,
    uint32_t voff, float (&acc)[32], int& bad) {
    using G = QuantGeom<4, LPR>;
    u32x4 buf[UU];
    uint32_t sc[UU];
    bool ok[UU];
#pragma unroll
    for (int u = 0; u < UU; ++u) {
        const uint32_t r = quant_slot<LPR, G::K>(myr, gbase, i0 + u);
        ok[u] = r != ~0u;
        const uint32_t row = ok[u] ? r : 0u;
        buf[u] = *reinterpret_cast<const u32x4*>(table + (uint64_t)row * ldb + voff);
        sc[u] = sbase[(uint64_t)row * sstride];
    }
#pragma unroll
    for (int u = 0; u < UU; ++u) {
        bad += ok[u] ? 0 : 1;
        const float s = mx4_scale_operand(ok[u] ? sc[u] : 0u);
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const uint32_t p = ok[u] ? buf[u][w] : 0u;
            const fp8_f32x2 v0 = ET_MX4_CVT(p, s, 0), v1 = ET_MX4_CVT(p, s, 1);
            const fp8_f32x2 v2 = ET_MX4_CVT(p, s, 2), v3 = ET_MX4_CVT(p, s, 3);
            float* a = acc + 8 * w;
            a[0] = a[0] + v0[0];
            a[1] = a[1] + v0[1];
            a[2] = a[2] + v1[0];
            a[3] = a[3] + v1[1];
            a[4] = a[4] + v2[0];
            a[5] = a[5] + v2[1];
            a[6] = a[6] + v3[0];
            a[7] = a[7] + v3[1];
        }
    }
}

// Vector kernel: grid = kXcds * ntables * stripe_chunks workgroups of 256; a workgroup owns
// 4 * GPW consecutive bags of one table.  `out` is the destination's ET_* element type.
template <int LPR>
__global__ ET_FP8_KERNEL __launch_bounds__(256) void k_mx4_vec(
    QuantPack pack, QuantStripes sm, int ntables, int64_t batch, void* __restrict__ dst,
    int64_t ld_dst, int out, int nt, int64_t stripe_chunks, int64_t nchunks) {
    using G = QuantGeom<4, LPR>;
    constexpr int F = 32, CH = G::CH, K = G::K, U = G::U;
    static_assert(G::F == F, "a lane owns one block of 32 features");
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
    const uint32_t payload = (uint32_t)d.dim / 2u;
    const int vpr = (int)(payload / 16u);  // blocks of the row
    const uint32_t blk = (uint32_t)(sub < vpr ? sub : vpr - 1);
    const uint32_t voff = 16u * blk;
    const uint8_t* sbase = (d.hdr ? reinterpret_cast<const uint8_t*>(d.hdr)
                                  : reinterpret_cast<const uint8_t*>(table) + payload) + blk;
    const uint32_t sstride = d.hdr ? mx4_hdr_stride((uint32_t)d.dim) : ldb;
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
#define ET_MX4_LOAD_ADD(UU, I0)                                                                \
    mx4_load_add<LPR, UU>(table, ldb, sbase, sstride, myr, gbase, I0, voff, acc, bad)
        int i0 = 0;
        if constexpr (K > 1) {
            // CH == U: a full chunk is one batch at compile-time slots
            if (cnt == CH) {
                ET_MX4_LOAD_ADD(U, 0);
                i0 = CH;
            }
        } else {
            for (; i0 + U <= cnt; i0 += U) ET_MX4_LOAD_ADD(U, i0);
        }
        if (cnt - i0 >= 4) {
            ET_MX4_LOAD_ADD(4, i0);
            i0 += 4;
        }
        if (cnt - i0 >= 2) {
            ET_MX4_LOAD_ADD(2, i0);
            i0 += 2;
        }
        if (cnt - i0 >= 1) ET_MX4_LOAD_ADD(1, i0);
#undef ET_MX4_LOAD_ADD
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

// Generic kernel: any alignment, leading dimension and payload size (byte reads only).  One
// wave per bag, lanes stride over the features, the bag's rows sequential per feature.
template <typename O>
__global__ ET_FP8_KERNEL __launch_bounds__(256) void k_mx4_generic(
    QuantPack pack, int ntables, int64_t batch, O* __restrict__ dst, int64_t ld_dst, int nt) {
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
    const int dim = d.dim;
    const uint32_t hstride = mx4_hdr_stride((uint32_t)dim);
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
            const uint8_t* h = hdr ? hdr + row * hstride : r + dim / 2;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const int f = f0 + lane + 64 * k;
                if (f < dim) {
                    // a zero row, not row 1's codes or its scale byte
                    const uint32_t byte = ok ? (uint32_t)r[f >> 1] : 0u;
                    const float s = mx4_scale_operand(ok ? (uint32_t)h[f >> 5] : 0u);
                    const fp8_f32x2 p = ET_MX4_CVT(byte, s, 0);
                    const float v = (f & 1) ? p[1] : p[0];
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

// Quantiser (not a hot path): work is split by block, a lane pair per block of 32 features, so
// a row of one block and a row of 64 keep a wave equally busy and amax is one exchange inside
// the pair.  A lane reads its 16 features, the pair agrees on
//   e = max(expfield(amax) - 2, 0)
// and each lane encodes its 8 payload bytes with v_cvt_scalef32_pk_fp4_f32 (x / 2^(e-127),
// saturated at +-6, rounded to nearest with ties to the even code: the contract's
// clamp-then-RNE, measured equal on every tie, both neighbours of every tie and subnormal
// inputs).  Byte stores only, so any alignment; writes the payload and the scale
// bytes, never the padding.
__global__ ET_FP8_KERNEL __launch_bounds__(256) void k_mx4_quantize_rows(
    const float* __restrict__ src, int64_t ld_src, int64_t nrows, int dim,
    uint8_t* __restrict__ table, int64_t ld_bytes, uint8_t* __restrict__ hdr) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int nb = dim / 32;
    const int64_t blk = t >> 1;
    const int half = (int)(t & 1);
    // a pair is two neighbouring lanes of one wave: both leave together
    if (blk >= nrows * nb) return;
    const int64_t row = blk / nb;
    const int b = (int)(blk % nb);
    const float* x = src + row * ld_src + 32 * b + 16 * half;
    float v[16];
    float amax = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        v[k] = x[k];
        amax = fmaxf(amax, fabsf(v[k]));
    }
    amax = fmaxf(amax, fp8_lane_xor(amax, threadIdx.x & 63, 1));
    const int ef = (int)((__builtin_bit_cast(uint32_t, amax) >> 23) & 0xffu);
    const uint32_t e = (uint32_t)(ef > 2 ? ef - 2 : 0);
    const float s = mx4_scale_operand(e);
    uint32_t w[2] = {0u, 0u};
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const float* y = v + 8 * q;
        w[q] = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(w[q], y[0], y[1], s, 0);
        w[q] = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(w[q], y[2], y[3], s, 1);
        w[q] = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(w[q], y[4], y[5], s, 2);
        w[q] = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(w[q], y[6], y[7], s, 3);
    }
    uint8_t* out = table + row * ld_bytes;
    uint8_t* p = out + 16 * b + 8 * half;
#pragma unroll
    for (int k = 0; k < 8; ++k) p[k] = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
    if (half == 0) {
        uint8_t* sc = hdr ? hdr + row * mx4_hdr_stride((uint32_t)dim) : out + dim / 2;
        sc[b] = (uint8_t)e;
    }
}

// ---------------------------------------------------------------------------
// Host dispatch
// ---------------------------------------------------------------------------

template <int LPR>
int launch_mx4_vec(const QuantPack& pack, int n, int64_t batch, void* dst, int64_t ld_dst, int out,
                   bool nt, hipStream_t s) {
    QuantGrid g;
    const int rc = quant_vec_grid(pack, n, batch, 4 * QuantGeom<4, LPR>::GPW, &g);
    if (rc != ET_OK) return rc;
    hipLaunchKernelGGL((k_mx4_vec<LPR>), dim3((unsigned)g.grid), dim3(256), 0, s, pack, g.sm, n,
                       batch, dst, ld_dst, out, nt ? 1 : 0, g.stripe_chunks, g.nchunks);
    ET_LAUNCH_CHECK("k_mx4_vec");
    return ET_OK;
}

inline int launch_mx4_vec_lpr(int lpr, const QuantPack& pack, int n, int64_t batch, void* dst,
                              int64_t ld_dst, int out, bool nt, hipStream_t s) {
    switch (lpr) {
        case 1: return launch_mx4_vec<1>(pack, n, batch, dst, ld_dst, out, nt, s);
        case 2: return launch_mx4_vec<2>(pack, n, batch, dst, ld_dst, out, nt, s);
        case 4: return launch_mx4_vec<4>(pack, n, batch, dst, ld_dst, out, nt, s);
        case 8: return launch_mx4_vec<8>(pack, n, batch, dst, ld_dst, out, nt, s);
        case 16: return launch_mx4_vec<16>(pack, n, batch, dst, ld_dst, out, nt, s);
        case 32: return launch_mx4_vec<32>(pack, n, batch, dst, ld_dst, out, nt, s);
        case 64: return launch_mx4_vec<64>(pack, n, batch, dst, ld_dst, out, nt, s);
    }
    return fail(ET_ERR_UNSUPPORTED, "MXFP4 vector lane group %d", lpr);
}

template <typename O>
int launch_mx4_generic(const QuantPack& pack, int n, int64_t batch, void* dst, int64_t ld_dst,
                       bool nt, hipStream_t s) {
    const int64_t grid = (batch + 3) / 4 * n;
    if (grid > 0x7fffffffll) return fail(ET_ERR_ARG, "grid too large");
    hipLaunchKernelGGL((k_mx4_generic<O>), dim3((unsigned)grid), dim3(256), 0, s, pack, n, batch,
                       reinterpret_cast<O*>(dst), ld_dst, nt ? 1 : 0);
    ET_LAUNCH_CHECK("k_mx4_generic");
    return ET_OK;
}

// quant_dispatch for MXFP4 rows: the INT entry's validation with bits pinned to 4, dim a
// multiple of 32 and a trailer of dim / 32 scale bytes, then one kernel per group of tables.
inline int mx4_dispatch(int out, const et_quant_desc* descs, int ntables, int64_t batch, void* dst,
                        int64_t ld_dst, uint32_t flags, hipStream_t s) {
    int key_of[ET_MAX_TABLES_PER_LAUNCH];
    bool work;
    const int rc =
        quant_validate(out, descs, ntables, batch, dst, ld_dst, flags, 4, key_of, &work, true);
    if (rc != ET_OK || !work) return rc;
    open_side_streams(s);
    const bool nt = (flags & ET_FLAG_NONTEMPORAL) != 0;
    return quant_for_groups(descs, ntables, key_of, [&](int key, const QuantPack& pack, int n) {
        if (key == 0)
            return out == ET_F32   ? launch_mx4_generic<float>(pack, n, batch, dst, ld_dst, nt, s)
                   : out == ET_F16 ? launch_mx4_generic<_Float16>(pack, n, batch, dst, ld_dst, nt, s)
                                   : launch_mx4_generic<__bf16>(pack, n, batch, dst, ld_dst, nt, s);
        return launch_mx4_vec_lpr(key % 256, pack, n, batch, dst, ld_dst, out, nt, s);
    });
}

}  // namespace et

extern "C" int et_mx4_quantize_rows(const float* src, int64_t ld_src, int64_t nrows, int32_t dim,
                                    void* table, int64_t ld_bytes, void* scales, void* stream) {
    et::clear_err();
    if (dim % 32 != 0)
        return et::fail(ET_ERR_ARG, "quantise: dim %d is not a multiple of 32 (one MXFP4 block)", dim);
    int64_t payload = 0;
    const int rc = et::quant_row_check("quantise", 0, dim, 4, ld_bytes, scales == nullptr, &payload,
                                       dim / 32);
    if (rc != ET_OK) return rc;
    if (nrows < 0) return et::fail(ET_ERR_ARG, "negative nrows");
    if (ld_src < dim) return et::fail(ET_ERR_ARG, "ld_src < dim");
    if (nrows == 0 || dim == 0) return ET_OK;
    if (!src || !table) return et::fail(ET_ERR_ARG, "NULL src/table");
    const int64_t grid = (nrows * (dim / 32) * 2 + 255) / 256;  // a lane pair per block
    if (grid > 0x7fffffffll) return et::fail(ET_ERR_ARG, "grid too large");
    hipStream_t s = static_cast<hipStream_t>(stream);
    et::open_side_streams(s);
    hipLaunchKernelGGL(et::k_mx4_quantize_rows, dim3((unsigned)grid), dim3(256), 0, s, src, ld_src,
                       nrows, (int)dim, static_cast<uint8_t*>(table), ld_bytes,
                       static_cast<uint8_t*>(scales));
    ET_LAUNCH_CHECK("k_mx4_quantize_rows");
    return ET_OK;
}

extern "C" int et_mx4_maplookup_prealloc(int dst_dtype, const et_quant_desc* descs, int32_t ntables,
                                         int64_t batch, void* dst, int64_t ld_dst, uint32_t flags,
                                         void* stream) {
    et::clear_err();
    return et::mx4_dispatch(dst_dtype, descs, ntables, batch, dst, ld_dst, flags,
                            static_cast<hipStream_t>(stream));
}
