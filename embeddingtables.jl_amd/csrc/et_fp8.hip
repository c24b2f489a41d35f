// et_fp8.hip — FP8 rows (OCP E4M3FN / E5M2, one code per feature, a Float16 scale and bias per
// row): the pooled lookup with the dequantisation fused into the sum, and the quantiser.
// Textually included behind et_quant.hip: the row layout, the descriptors, the bag and index
// plumbing (quant_bag, quant_slot, QuantGeom<8, LPR>, quant_store), the stripe schedule and the
// host validation are that file's; only the decode, the out-of-range rule and the quantiser's
// arithmetic differ.  The format and the arithmetic are defined in include/embtab.h.
//
//   * v = float(q) * float(scale) + float(bias): an FP8 value has at most 4 significant bits and
//     a half 11, the product is exact, so one fma per feature is the one rounding of the contract.
//   * Decode is the hardware's: v_cvt_pk_f32_fp8 / v_cvt_pk_f32_bf8 turn the low or the high
//     half of a payload word into two Float32 values, so a lane's 16 features are eight
//     conversions (INT8: sixteen).  The format is a template parameter.
//   * An out-of-range index must add +0 whatever row 1 holds, and a NaN or Inf code times a zero
//     scale is NaN: the lane replaces the payload AND the header of such a row by zeros (code 0 is
//     +0 in both formats; fma(+0, +0, +0) = +0).
//   * The kernels here opt out of packed Float32 arithmetic (v_pk_fma_f32 / v_pk_add_f32): every
//     result is pinned bit for bit, and the fma and the add are issued one feature at a time.
//
// Vector kernel: k_quant_vec's geometry for 8-bit rows (a lane owns 16 payload bytes, LPR lanes
// a bag, 64 / LPR bags a wave, eight rows of a group in flight, each a 16-byte payload load and
// a 4-byte header load); see DESIGN for why the depth stays at eight.

namespace et {

#if defined(__HIP_DEVICE_COMPILE__)
#define ET_FP8_KERNEL __attribute__((target("no-packed-fp32-ops")))
#else
#define ET_FP8_KERNEL
#endif

typedef float fp8_f32x2 __attribute__((ext_vector_type(2)));

// Bytes 0-1 (HI = false) or 2-3 (HI = true) of `w` as two Float32 values.
template <int FMT, bool HI>
__device__ __forceinline__ fp8_f32x2 fp8_decode2(uint32_t w) {
    if constexpr (FMT == ET_FP8_E4M3)
        return __builtin_amdgcn_cvt_pk_f32_fp8((int)w, HI);
    else
        return __builtin_amdgcn_cvt_pk_f32_bf8((int)w, HI);
}

// The 16 payload bytes of a lane as 16 Float32 values, in feature order.
template <int FMT>
__device__ __forceinline__ void fp8_unpack(u32x4 p, float (&q)[16]) {
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const fp8_f32x2 lo = fp8_decode2<FMT, false>(p[w]), hi = fp8_decode2<FMT, true>(p[w]);
        q[4 * w] = lo[0];
        q[4 * w + 1] = lo[1];
        q[4 * w + 2] = hi[0];
        q[4 * w + 3] = hi[1];
    }
}

// quant_load_add for FP8 rows: UU rows of one bag (slots i0 .. i0+UU-1, all valid), every load
// issued before the first row is consumed, the rows added in slot order onto accumulators that
// start at -0.0.  An out-of-range slot loads row 0 and is then replaced by a zero payload and a
// zero header.
template <int FMT, int LPR, int UU>
__device__ __forceinline__ void fp8_load_add(
    const char* __restrict__ table, uint32_t ldb, const char* __restrict__ hbase, uint32_t hstride,
    const uint32_t (&myr)[QuantGeom<8, LPR>::K], int gbase, int i0, uint32_t voff,
    float (&acc)[16], int& bad) {
    using G = QuantGeom<8, LPR>;
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
        u32x4 p;
#pragma unroll
        for (int w = 0; w < 4; ++w) p[w] = ok[u] ? buf[u][w] : 0u;
        const float s = half_bits_f32(h & 0xffffu), b = half_bits_f32(h >> 16);
        float q[16];
        fp8_unpack<FMT>(p, q);
#pragma unroll
        for (int f = 0; f < 16; ++f) {
            const float v = __builtin_fmaf(q[f], s, b);  // exact product: one rounding
            acc[f] = acc[f] + v;
        }
    }
}

// Vector kernel: grid = kXcds * ntables * stripe_chunks workgroups of 256; a workgroup owns
// 4 * GPW consecutive bags of one table.  `out` is the destination's ET_* element type.
template <int FMT, int LPR>
__global__ ET_FP8_KERNEL __launch_bounds__(256) void k_fp8_vec(
    QuantPack pack, QuantStripes sm, int ntables, int64_t batch, void* __restrict__ dst,
    int64_t ld_dst, int out, int nt, int64_t stripe_chunks, int64_t nchunks) {
    using G = QuantGeom<8, LPR>;
    constexpr int F = 16, CH = G::CH, K = G::K, U = G::U;
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
    const uint32_t payload = (uint32_t)d.dim;
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
#define ET_FP8_LOAD_ADD(UU, I0)                                                                \
    fp8_load_add<FMT, LPR, UU>(table, ldb, hbase, hstride, myr, gbase, I0, voff, acc, bad)
        int i0 = 0;
        if constexpr (K > 1) {
            // CH == U: a full chunk is one batch at compile-time slots
            if (cnt == CH) {
                ET_FP8_LOAD_ADD(U, 0);
                i0 = CH;
            }
        } else {
            for (; i0 + U <= cnt; i0 += U) ET_FP8_LOAD_ADD(U, i0);
        }
        if (cnt - i0 >= 4) {
            ET_FP8_LOAD_ADD(4, i0);
            i0 += 4;
        }
        if (cnt - i0 >= 2) {
            ET_FP8_LOAD_ADD(2, i0);
            i0 += 2;
        }
        if (cnt - i0 >= 1) ET_FP8_LOAD_ADD(1, i0);
#undef ET_FP8_LOAD_ADD
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
template <typename O, int FMT>
__global__ ET_FP8_KERNEL __launch_bounds__(256) void k_fp8_generic(
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
            const uint8_t* h = hdr ? hdr + row * 4u : r + dim;
            const float s = ok ? half_bits_f32((uint32_t)h[0] | ((uint32_t)h[1] << 8)) : 0.f;
            const float b = ok ? half_bits_f32((uint32_t)h[2] | ((uint32_t)h[3] << 8)) : 0.f;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const int f = f0 + lane + 64 * k;
                if (f < dim) {
                    const uint32_t code = ok ? (uint32_t)r[f] : 0u;  // a zero row, not row 1's codes
                    const float v = __builtin_fmaf(fp8_decode2<FMT, false>(code)[0], s, b);
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

// x of lane (lane ^ m) of the wave.
__device__ __forceinline__ float fp8_lane_xor(float x, int lane, int m) {
    return __builtin_bit_cast(
        float, __builtin_amdgcn_ds_bpermute((lane ^ m) << 2, __builtin_bit_cast(int, x)));
}

// Quantiser (not a hot path): one wave per row, include/embtab.h's arithmetic.  The quotient is
// clamped to +-FMAX in Float32 and then rounded once by the hardware conversion (nearest even;
// a clamped input never reaches its saturation or NaN rules).  Byte stores only, so any
// alignment; writes the payload and the header, never the padding.
template <int FMT>
__global__ ET_FP8_KERNEL __launch_bounds__(256) void k_fp8_quantize_rows(
    const float* __restrict__ src, int64_t ld_src, int64_t nrows, int dim,
    uint8_t* __restrict__ table, int64_t ld_bytes, uint8_t* __restrict__ hdr) {
    constexpr float FMAX = FMT == ET_FP8_E4M3 ? 448.f : 57344.f;
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
        lo = fminf(lo, fp8_lane_xor(lo, lane, m));
        hi = fmaxf(hi, fp8_lane_xor(hi, lane, m));
    }
    // opaque Float32 results: each is rounded to Float32 and then to half, never folded into one
    // mix-to-half instruction
    float mid = (lo + hi) / 2.f;
    asm("" : "+v"(mid));
    _Float16 bh = (_Float16)mid;
    const float b = (float)bh;
    float sc = fmaxf(hi - b, b - lo) / FMAX;
    asm("" : "+v"(sc));
    _Float16 sh = (_Float16)sc;
    float s = (float)sh;
    if (!(s > 0.f && s < __builtin_inff())) {
        sh = (_Float16)1.0f;
        s = 1.0f;
    }
    uint8_t* out = table + row * ld_bytes;
    for (int f = lane; f < dim; f += 64) {
        const float c = fminf(fmaxf((x[f] - b) / s, -FMAX), FMAX);
        int code;
        if constexpr (FMT == ET_FP8_E4M3)
            code = __builtin_amdgcn_cvt_pk_fp8_f32(c, c, 0, false);
        else
            code = __builtin_amdgcn_cvt_pk_bf8_f32(c, c, 0, false);
        out[f] = (uint8_t)(code & 0xff);
    }
    if (lane == 0) {
        uint16_t su, bu;
        __builtin_memcpy(&su, &sh, 2);
        __builtin_memcpy(&bu, &bh, 2);
        uint8_t* h = hdr ? hdr + row * 4 : out + dim;
        h[0] = (uint8_t)(su & 0xff);
        h[1] = (uint8_t)(su >> 8);
        h[2] = (uint8_t)(bu & 0xff);
        h[3] = (uint8_t)(bu >> 8);
    }
}

// ---------------------------------------------------------------------------
// Host dispatch
// ---------------------------------------------------------------------------

inline bool fp8_format_ok(int format) { return format == ET_FP8_E4M3 || format == ET_FP8_E5M2; }

template <int FMT, int LPR>
int launch_fp8_vec(const QuantPack& pack, int n, int64_t batch, void* dst, int64_t ld_dst, int out,
                   bool nt, hipStream_t s) {
    QuantGrid g;
    const int rc = quant_vec_grid(pack, n, batch, 4 * QuantGeom<8, LPR>::GPW, &g);
    if (rc != ET_OK) return rc;
    hipLaunchKernelGGL((k_fp8_vec<FMT, LPR>), dim3((unsigned)g.grid), dim3(256), 0, s, pack, g.sm,
                       n, batch, dst, ld_dst, out, nt ? 1 : 0, g.stripe_chunks, g.nchunks);
    ET_LAUNCH_CHECK("k_fp8_vec");
    return ET_OK;
}

template <int FMT>
int launch_fp8_vec_fmt(int lpr, const QuantPack& pack, int n, int64_t batch, void* dst,
                       int64_t ld_dst, int out, bool nt, hipStream_t s) {
    switch (lpr) {
        case 1: return launch_fp8_vec<FMT, 1>(pack, n, batch, dst, ld_dst, out, nt, s);
        case 2: return launch_fp8_vec<FMT, 2>(pack, n, batch, dst, ld_dst, out, nt, s);
        case 4: return launch_fp8_vec<FMT, 4>(pack, n, batch, dst, ld_dst, out, nt, s);
        case 8: return launch_fp8_vec<FMT, 8>(pack, n, batch, dst, ld_dst, out, nt, s);
        case 16: return launch_fp8_vec<FMT, 16>(pack, n, batch, dst, ld_dst, out, nt, s);
        case 32: return launch_fp8_vec<FMT, 32>(pack, n, batch, dst, ld_dst, out, nt, s);
        case 64: return launch_fp8_vec<FMT, 64>(pack, n, batch, dst, ld_dst, out, nt, s);
    }
    return fail(ET_ERR_UNSUPPORTED, "FP8 vector lane group %d", lpr);
}

template <typename O, int FMT>
int launch_fp8_generic(const QuantPack& pack, int n, int64_t batch, void* dst, int64_t ld_dst,
                       bool nt, hipStream_t s) {
    const int64_t grid = (batch + 3) / 4 * n;
    if (grid > 0x7fffffffll) return fail(ET_ERR_ARG, "grid too large");
    hipLaunchKernelGGL((k_fp8_generic<O, FMT>), dim3((unsigned)grid), dim3(256), 0, s, pack, n,
                       batch, reinterpret_cast<O*>(dst), ld_dst, nt ? 1 : 0);
    ET_LAUNCH_CHECK("k_fp8_generic");
    return ET_OK;
}

// quant_dispatch for one FP8 format: the INT entry's validation with bits pinned to 8, then one
// kernel per group of tables (generic, or the vector kernel of a lane-group capacity).
template <int FMT>
int fp8_dispatch(int out, const et_quant_desc* descs, int ntables, int64_t batch, void* dst,
                 int64_t ld_dst, uint32_t flags, hipStream_t s) {
    int key_of[ET_MAX_TABLES_PER_LAUNCH];
    bool work;
    const int rc = quant_validate(out, descs, ntables, batch, dst, ld_dst, flags, 8, key_of, &work);
    if (rc != ET_OK || !work) return rc;
    open_side_streams(s);
    const bool nt = (flags & ET_FLAG_NONTEMPORAL) != 0;
    return quant_for_groups(descs, ntables, key_of, [&](int key, const QuantPack& pack, int n) {
        if (key == 0)
            return out == ET_F32   ? launch_fp8_generic<float, FMT>(pack, n, batch, dst, ld_dst, nt, s)
                   : out == ET_F16 ? launch_fp8_generic<_Float16, FMT>(pack, n, batch, dst, ld_dst, nt, s)
                                   : launch_fp8_generic<__bf16, FMT>(pack, n, batch, dst, ld_dst, nt, s);
        return launch_fp8_vec_fmt<FMT>(key % 256, pack, n, batch, dst, ld_dst, out, nt, s);
    });
}

template <int FMT>
void launch_fp8_quantize(int64_t grid, hipStream_t s, const float* src, int64_t ld_src,
                         int64_t nrows, int dim, void* table, int64_t ld_bytes, void* hdr) {
    hipLaunchKernelGGL(k_fp8_quantize_rows<FMT>, dim3((unsigned)grid), dim3(256), 0, s, src, ld_src,
                       nrows, dim, static_cast<uint8_t*>(table), ld_bytes,
                       static_cast<uint8_t*>(hdr));
}

}  // namespace et

extern "C" int et_fp8_quantize_rows(int format, const float* src, int64_t ld_src, int64_t nrows,
                                    int32_t dim, void* table, int64_t ld_bytes, void* hdr,
                                    void* stream) {
    et::clear_err();
    if (!et::fp8_format_ok(format))
        return et::fail(ET_ERR_UNSUPPORTED, "FP8 format %d is neither 1 (E4M3) nor 2 (E5M2)", format);
    int64_t payload = 0;
    const int rc = et::quant_row_check("quantise", 0, dim, 8, ld_bytes, hdr == nullptr, &payload);
    if (rc != ET_OK) return rc;
    if (nrows < 0) return et::fail(ET_ERR_ARG, "negative nrows");
    if (ld_src < dim) return et::fail(ET_ERR_ARG, "ld_src < dim");
    if (nrows == 0 || dim == 0) return ET_OK;
    if (!src || !table) return et::fail(ET_ERR_ARG, "NULL src/table");
    const int64_t grid = (nrows + 3) / 4;
    if (grid > 0x7fffffffll) return et::fail(ET_ERR_ARG, "grid too large");
    hipStream_t s = static_cast<hipStream_t>(stream);
    et::open_side_streams(s);
    if (format == ET_FP8_E4M3)
        et::launch_fp8_quantize<ET_FP8_E4M3>(grid, s, src, ld_src, nrows, dim, table, ld_bytes, hdr);
    else
        et::launch_fp8_quantize<ET_FP8_E5M2>(grid, s, src, ld_src, nrows, dim, table, ld_bytes, hdr);
    ET_LAUNCH_CHECK("k_fp8_quantize_rows");
    return ET_OK;
}

extern "C" int et_fp8_maplookup_prealloc(int dst_dtype, int format, const et_quant_desc* descs,
                                         int32_t ntables, int64_t batch, void* dst, int64_t ld_dst,
                                         uint32_t flags, void* stream) {
    et::clear_err();
    if (!et::fp8_format_ok(format))
        return et::fail(ET_ERR_UNSUPPORTED, "FP8 format %d is neither 1 (E4M3) nor 2 (E5M2)", format);
    hipStream_t s = static_cast<hipStream_t>(stream);
    return format == ET_FP8_E4M3
               ? et::fp8_dispatch<ET_FP8_E4M3>(dst_dtype, descs, ntables, batch, dst, ld_dst, flags, s)
               : et::fp8_dispatch<ET_FP8_E5M2>(dst_dtype, descs, ntables, batch, dst, ld_dst, flags, s);
}
