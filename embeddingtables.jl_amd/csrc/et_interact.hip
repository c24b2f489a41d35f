// et_interact.hip — the DLRM pairwise dot interaction on the matrix units, forward and
// backward (include/embtab.h, "Pairwise dot interaction"; DESIGN.md §"Dot interaction").
// Textually included from et_misc.hip.
//
// One wave owns one sample at a time: its F x F product is one 32x32 MFMA tile (F <= 32), so
// nothing is ever summed across waves and a sample's bits depend on (T, F, D) alone.  A
// workgroup is ET_INTERACT_WAVES independent waves (no workgroup barrier anywhere); the grid
// is capped at ET_INTERACT_GRID_CAP workgroups and strides over the batch.

namespace et {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned short u16x8 __attribute__((ext_vector_type(8)));
typedef unsigned short u16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

constexpr int kIxWaves = ET_INTERACT_WAVES;
constexpr int kIxRowB = 144;              // a staged row chunk: 128 bytes + 16 of padding
constexpr int kIxStageB = 32 * kIxRowB;   // 32 rows; also holds the 528-float triangle

// Orders this wave's LDS traffic: what its lanes wrote before is what they read after.
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// acc += A(32x16) * B(16x32) for a 16-bit T: lane (l%32, l/32) holds 8 consecutive k.
template <typename T>
__device__ __forceinline__ f32x16 mfma16(u16x8 a, u16x8 b, f32x16 acc) {
    if constexpr (__is_same(T, __bf16))
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a),
                                                       __builtin_bit_cast(bf16x8, b), acc, 0, 0, 0);
    else
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a),
                                                      __builtin_bit_cast(f16x8, b), acc, 0, 0, 0);
}

template <typename T>
struct IxBits {
    typedef uint16_t type;
};
template <>
struct IxBits<float> {
    typedef uint32_t type;
};

// ---------------------------------------------------------------------------------------
// Forward: Z = X Xt.  The sample's rows are staged through LDS in chunks of 128 bytes a row:
// the global loads are coalesced (8 lanes cover a row chunk, a full cache line), the LDS
// reads hand lane (i = l%32, h = l/32) the 16-byte piece 2*step + h of row i.  With B = At
// that one register is both MFMA operands, and since the result is a sum over k any
// assignment of pieces to (h, step) is valid.  Rows >= F and pieces behind the row are never
// loaded: their slots are stored as zeros.  The next chunk's global loads are issued before
// the MFMAs of the current one.
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ void ix_load_chunk(const char* __restrict__ xs, int ch, int F,
                                              int row_b, int npieces, int lane, u32x4 (&g)[4]) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int slot = lane + 64 * u, r = slot >> 3, p = ch * 8 + (slot & 7);
        const u32x4 zero = {0, 0, 0, 0};
        g[u] = zero;
        if (r < F && p < npieces)
            g[u] = *reinterpret_cast<const u32x4*>(xs + (int64_t)r * row_b + p * 16);
    }
}

template <typename T, bool ITSELF, bool NT>
__global__ __launch_bounds__(64 * kIxWaves) __attribute__((amdgpu_waves_per_eu(4, 8))) void k_interact_fwd(
    const char* __restrict__ x, int64_t ldx_b, int64_t batch, int F, int row_b, int copy,
    char* __restrict__ y, int64_t ldy_b) {
    __shared__ __attribute__((aligned(16))) char lds_all[kIxWaves][kIxStageB];
    typedef typename IxBits<T>::type Bits;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int i = lane & 31, h = lane >> 5;
    char* lds = lds_all[wave];
    const int npieces = row_b >> 4, nchunks = (npieces + 7) >> 3;
    const int NP = ITSELF ? F * (F + 1) / 2 : F * (F - 1) / 2;
    for (int64_t s = (int64_t)blockIdx.x * kIxWaves + wave; s < batch;
         s += (int64_t)gridDim.x * kIxWaves) {
        const char* xs = x + s * ldx_b;
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        u32x4 g[4];
        ix_load_chunk(xs, 0, F, row_b, npieces, lane, g);
        for (int ch = 0; ch < nchunks; ++ch) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int slot = lane + 64 * u;
                *reinterpret_cast<u32x4*>(lds + (slot >> 3) * kIxRowB + (slot & 7) * 16) = g[u];
            }
            wave_sync();
            if (ch + 1 < nchunks) ix_load_chunk(xs, ch + 1, F, row_b, npieces, lane, g);
#pragma unroll
            for (int st = 0; st < 4; ++st) {
                if (ch * 8 + 2 * st < npieces) {  // wave-uniform: a step wholly behind the row
                    const u32x4 v =
                        *reinterpret_cast<const u32x4*>(lds + i * kIxRowB + (2 * st + h) * 16);
                    if constexpr (sizeof(T) == 4) {
                        const f32x4 f = __builtin_bit_cast(f32x4, v);
#pragma unroll
                        for (int c = 0; c < 4; ++c)
                            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(f[c], f[c], acc, 0, 0, 0);
                    } else {
                        const u16x8 p = __builtin_bit_cast(u16x8, v);
                        acc = mfma16<T>(p, p, acc);
                    }
                }
            }
            wave_sync();  // the reads are done before the next chunk (or the triangle) lands
        }
        // The accumulator tile: column l%32, rows 8*(r/4) + 4*(l/32) + r%4.  The triangle goes
        // through LDS so that the sample's NP values leave as contiguous stores.
        float* tri = reinterpret_cast<float*>(lds);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int ii = 8 * (r >> 2) + 4 * h + (r & 3);
            if (ii < F && (i < ii || (ITSELF && i == ii)))
                tri[(ITSELF ? ii * (ii + 1) / 2 : ii * (ii - 1) / 2) + i] = acc[r];
        }
        wave_sync();
        T* ys = reinterpret_cast<T*>(y + s * ldy_b);
        for (int t = lane; t < NP; t += 64) store_scalar<NT, T>(ys + copy + t, (T)tri[t]);
        const Bits* xb = reinterpret_cast<const Bits*>(xs);
        Bits* yb = reinterpret_cast<Bits*>(ys);
        for (int t = lane; t < copy; t += 64) store_scalar<NT, Bits>(yb + t, xb[t]);
        wave_sync();  // the triangle is read before the next sample's first chunk lands
    }
}

// ---------------------------------------------------------------------------------------
// Backward: dX = G X, G the symmetric fill of the sample's NP gradient values (zero on the
// diagonal, or 2 G[i,i] with ITSELF), built once per sample in LDS and kept as the A operand
// in registers (K = F padded to 32).  X is the B operand with lanes along the features: lane
// (q = l%32, h = l/32) loads 4 consecutive features of row j = k, so 32 lanes cover a
// contiguous 512 (Float32) or 256 (16-bit) bytes of the row, and the 4 components feed 4
// accumulator tiles (tile c owns feature n0 + 4q + c).  D is walked in blocks of 128 columns.
// The output tile has registers along i, so a row of dX leaves as the same contiguous vectors.
// ---------------------------------------------------------------------------------------
template <typename T, bool ITSELF, bool NT>
__global__ __launch_bounds__(64 * kIxWaves) __attribute__((amdgpu_waves_per_eu(2, 8))) void k_interact_bwd(
    const char* __restrict__ x, int64_t ldx_b, const char* __restrict__ dy, int64_t lddy_b,
    int64_t batch, int F, int D, int copy, char* __restrict__ dx, int64_t lddx_b) {
    constexpr bool F32 = sizeof(T) == 4;
    constexpr bool DIAG_PASS = ITSELF && __is_same(T, _Float16);  // 2*g can overflow Float16
    typedef typename IxBits<T>::type Bits;
    constexpr int GS = F32 ? 33 : 40;  // row stride of G in elements (16-bit: 80 bytes)
    __shared__ __attribute__((aligned(16))) Bits g_all[kIxWaves][32 * GS];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int q = lane & 31, h = lane >> 5;
    Bits* G = g_all[wave];
    for (int64_t s = (int64_t)blockIdx.x * kIxWaves + wave; s < batch;
         s += (int64_t)gridDim.x * kIxWaves) {
        const T* dys = reinterpret_cast<const T*>(dy + s * lddy_b);
        const T* xs = reinterpret_cast<const T*>(x + s * ldx_b);
        T* dxs = reinterpret_cast<T*>(dx + s * lddx_b);
        // every cell of G is written once, by the lane that owns it: no clearing pass
#pragma unroll 4
        for (int it = 0; it < 16; ++it) {
            const int ii = 2 * it + h;
            T v = (T)0.f;
            if (ii < F && q < F) {
                const int hi = ii > q ? ii : q, lo = ii > q ? q : ii;
                if (hi != lo) {
                    v = dys[copy + (ITSELF ? hi * (hi + 1) / 2 : hi * (hi - 1) / 2) + lo];
                } else if (ITSELF) {
                    v = dys[copy + ii * (ii + 1) / 2 + ii];
                    if (!DIAG_PASS) v = (T)(2.f * (float)v);  // exact: a power of two
                }
            }
            G[ii * GS + q] = __builtin_bit_cast(Bits, v);
        }
        wave_sync();
        float a32[16];
        u16x8 a16[2], ad16[2];
        if constexpr (F32) {
#pragma unroll
            for (int t = 0; t < 16; ++t)
                a32[t] = __builtin_bit_cast(float, (uint32_t)G[q * GS + 2 * t + h]);
        } else {
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                a16[t] = *reinterpret_cast<const u16x8*>(&G[q * GS + 16 * t + 8 * h]);
                if constexpr (DIAG_PASS) {
                    const Bits gd = G[q * GS + q];
#pragma unroll
                    for (int e = 0; e < 8; ++e) ad16[t][e] = (16 * t + 8 * h + e == q) ? gd : 0;
                }
            }
        }
        wave_sync();  // G is in registers: the next sample may overwrite it
        for (int n0 = 0; n0 < D; n0 += 128) {
            const int n = n0 + 4 * q;
            const bool cv = n < D;
            f32x16 acc[4];
#pragma unroll
            for (int c = 0; c < 4; ++c)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[c][r] = 0.f;
            if constexpr (F32) {
#pragma unroll
                for (int half = 0; half < 2; ++half) {
                    if (16 * half < F) {
                        f32x4 xv[8];
#pragma unroll
                        for (int u = 0; u < 8; ++u) {
                            const int j = 2 * (8 * half + u) + h;
                            const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
                            xv[u] = zero;
                            if (cv && j < F)
                                xv[u] = *reinterpret_cast<const f32x4*>(xs + (int64_t)j * D + n);
                        }
#pragma unroll
                        for (int u = 0; u < 8; ++u) {
                            if (2 * (8 * half + u) < F) {
#pragma unroll
                                for (int c = 0; c < 4; ++c)
                                    acc[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(
                                        a32[8 * half + u], xv[u][c], acc[c], 0, 0, 0);
                            }
                        }
                    }
                    __builtin_amdgcn_sched_barrier(0);  // keep the second half's loads behind
                }
            } else {
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    if (16 * t < F) {
                        u16x4 w[8];
#pragma unroll
                        for (int e = 0; e < 8; ++e) {
                            const int j = 16 * t + 8 * h + e;
                            const u16x4 zero = {0, 0, 0, 0};
                            w[e] = zero;
                            if (cv && j < F)
                                w[e] = *reinterpret_cast<const u16x4*>(xs + (int64_t)j * D + n);
                        }
#pragma unroll
                        for (int c = 0; c < 4; ++c) {
                            u16x8 b;
#pragma unroll
                            for (int e = 0; e < 8; ++e) b[e] = w[e][c];
                            acc[c] = mfma16<T>(a16[t], b, acc[c]);
                            if constexpr (DIAG_PASS) acc[c] = mfma16<T>(ad16[t], b, acc[c]);
                        }
                    }
                    __builtin_amdgcn_sched_barrier(0);  // keep the second step's loads behind
                }
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ii = 8 * (r >> 2) + 4 * h + (r & 3);
                if (ii < F && cv) {
                    const int flat = ii * D + n;
                    float o[4];
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        o[c] = acc[c][r];
                        if (flat + c < copy) o[c] = o[c] + (float)dys[flat + c];
                    }
                    if constexpr (F32) {
                        const f32x4 ov = {o[0], o[1], o[2], o[3]};
                        store16<NT>(dxs + flat, __builtin_bit_cast(u32x4, ov));
                    } else {
                        u16x4 ov;
#pragma unroll
                        for (int c = 0; c < 4; ++c) ov[c] = __builtin_bit_cast(uint16_t, (T)o[c]);
                        if constexpr (NT)
                            __builtin_nontemporal_store(ov, reinterpret_cast<u16x4*>(dxs + flat));
                        else
                            *reinterpret_cast<u16x4*>(dxs + flat) = ov;
                    }
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------------------
// Everything both entries check before a launch; *done is set for a successful no-op.
inline int interact_check(int dtype, int64_t batch, int32_t nvec, int32_t dim, int32_t copy,
                          uint32_t flags, bool* done) {
    *done = false;
    if (dtype != ET_F32 && dtype != ET_F16 && dtype != ET_BF16)
        return fail(ET_ERR_UNSUPPORTED, "interact: dtype %d (Float32, Float16, BFloat16)", dtype);
    if (flags & ~(ET_FLAG_NONTEMPORAL | ET_FLAG_INTERACT_ITSELF))
        return fail(ET_ERR_UNSUPPORTED, "interact: flags 0x%x", flags);
    if (nvec < 1 || nvec > ET_INTERACT_MAX_VECTORS)
        return fail(ET_ERR_UNSUPPORTED, "interact: nvec %d outside 1..%d", nvec,
                    ET_INTERACT_MAX_VECTORS);
    if (dim < 1 || dim > ET_INTERACT_MAX_DIM || (dim * elsize(dtype)) % 16)
        return fail(ET_ERR_UNSUPPORTED,
                    "interact: dim %d (dim * sizeof(T) a multiple of 16, dim <= %d)", dim,
                    ET_INTERACT_MAX_DIM);
    if (batch < 0) return fail(ET_ERR_ARG, "interact: negative batch");
    if (copy < 0 || copy > nvec * dim)
        return fail(ET_ERR_ARG, "interact: copy %d outside 0..%d", copy, nvec * dim);
    *done = batch == 0;
    return ET_OK;
}

inline bool ix_overlap(const void* a, int64_t a_bytes, const void* b, int64_t b_bytes) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + (uintptr_t)b_bytes && pb < pa + (uintptr_t)a_bytes;
}

inline int64_t ix_span(int64_t batch, int64_t ld, int64_t width, int es) {
    return ((batch - 1) * ld + width) * es;
}

inline unsigned ix_grid(int64_t batch) {
    const int64_t blocks = (batch + kIxWaves - 1) / kIxWaves;
    return (unsigned)(blocks < ET_INTERACT_GRID_CAP ? blocks : ET_INTERACT_GRID_CAP);
}

#define ET_IX_DISPATCH(KERNEL, ...)                                                        \
    do {                                                                                   \
        const bool it_ = flags & ET_FLAG_INTERACT_ITSELF, nt_ = flags & ET_FLAG_NONTEMPORAL; \
        const dim3 grid_(ix_grid(batch)), block_(64 * kIxWaves);                           \
        hipStream_t st_ = static_cast<hipStream_t>(stream);                                \
        if (it_ && nt_)                                                                    \
            hipLaunchKernelGGL((KERNEL<T, true, true>), grid_, block_, 0, st_, __VA_ARGS__); \
        else if (it_)                                                                      \
            hipLaunchKernelGGL((KERNEL<T, true, false>), grid_, block_, 0, st_, __VA_ARGS__); \
        else if (nt_)                                                                      \
            hipLaunchKernelGGL((KERNEL<T, false, true>), grid_, block_, 0, st_, __VA_ARGS__); \
        else                                                                               \
            hipLaunchKernelGGL((KERNEL<T, false, false>), grid_, block_, 0, st_, __VA_ARGS__); \
    } while (0)

template <typename T>
void interact_fwd_launch(const void* x, int64_t ld_x, int64_t batch, int F, int D, int copy,
                         void* y, int64_t ld_y, uint32_t flags, void* stream) {
    const int es = sizeof(T);
    ET_IX_DISPATCH(k_interact_fwd, static_cast<const char*>(x), ld_x * es, batch, F, D * es, copy,
                   static_cast<char*>(y), ld_y * es);
}

template <typename T>
void interact_bwd_launch(const void* x, int64_t ld_x, const void* dy, int64_t ld_dy,
                         int64_t batch, int F, int D, int copy, void* dx, int64_t ld_dx,
                         uint32_t flags, void* stream) {
    const int es = sizeof(T);
    ET_IX_DISPATCH(k_interact_bwd, static_cast<const char*>(x), ld_x * es,
                   static_cast<const char*>(dy), ld_dy * es, batch, F, D, copy,
                   static_cast<char*>(dx), ld_dx * es);
}

}  // namespace et

extern "C" int et_interact(int dtype, const void* x, int64_t ld_x, int64_t batch, int32_t nvec,
                           int32_t dim, int32_t copy, void* y, int64_t ld_y, uint32_t flags,
                           void* stream) {
    et::clear_err();
    et::open_side_streams(static_cast<hipStream_t>(stream));
    bool done;
    const int st = et::interact_check(dtype, batch, nvec, dim, copy, flags, &done);
    if (st != ET_OK || done) return st;
    const int es = et::elsize(dtype);
    const int64_t width = (int64_t)nvec * dim;
    const int64_t np = (flags & ET_FLAG_INTERACT_ITSELF) ? nvec * (nvec + 1) / 2
                                                         : nvec * (nvec - 1) / 2;
    if (!x || !y) return et::fail(ET_ERR_ARG, "interact: NULL argument");
    if (ld_x < width || ld_y < copy + np)
        return et::fail(ET_ERR_ARG, "interact: ld_x %lld < %lld or ld_y %lld < %lld",
                        (long long)ld_x, (long long)width, (long long)ld_y, (long long)(copy + np));
    if (!et::aligned16(x) || (ld_x * es) % 16)
        return et::fail(ET_ERR_UNSUPPORTED, "interact: the rows of x must be 16-byte aligned");
    if ((uintptr_t)y % es) return et::fail(ET_ERR_ARG, "interact: y is not aligned to its type");
    if (et::ix_overlap(x, et::ix_span(batch, ld_x, width, es), y,
                       et::ix_span(batch, ld_y, copy + np, es)))
        return et::fail(ET_ERR_ARG, "interact: y overlaps x");
    switch (dtype) {
        case ET_F32:
            et::interact_fwd_launch<float>(x, ld_x, batch, nvec, dim, copy, y, ld_y, flags, stream);
            break;
        case ET_F16:
            et::interact_fwd_launch<_Float16>(x, ld_x, batch, nvec, dim, copy, y, ld_y, flags,
                                              stream);
            break;
        default:
            et::interact_fwd_launch<__bf16>(x, ld_x, batch, nvec, dim, copy, y, ld_y, flags,
                                            stream);
    }
    ET_LAUNCH_CHECK("k_interact_fwd");
    return ET_OK;
}

extern "C" int et_interact_backward(int dtype, const void* x, int64_t ld_x, const void* dy,
                                    int64_t ld_dy, int64_t batch, int32_t nvec, int32_t dim,
                                    int32_t copy, void* dx, int64_t ld_dx, uint32_t flags,
                                    void* stream) {
    et::clear_err();
    et::open_side_streams(static_cast<hipStream_t>(stream));
    bool done;
    const int st = et::interact_check(dtype, batch, nvec, dim, copy, flags, &done);
    if (st != ET_OK || done) return st;
    const int es = et::elsize(dtype);
    const int64_t width = (int64_t)nvec * dim;
    const int64_t np = (flags & ET_FLAG_INTERACT_ITSELF) ? nvec * (nvec + 1) / 2
                                                         : nvec * (nvec - 1) / 2;
    if (!x || !dy || !dx) return et::fail(ET_ERR_ARG, "interact: NULL argument");
    if (ld_x < width || ld_dx < width || ld_dy < copy + np)
        return et::fail(ET_ERR_ARG, "interact: ld_x %lld or ld_dx %lld < %lld, or ld_dy %lld < %lld",
                        (long long)ld_x, (long long)ld_dx, (long long)width, (long long)ld_dy,
                        (long long)(copy + np));
    if (!et::aligned16(x) || (ld_x * es) % 16 || !et::aligned16(dx) || (ld_dx * es) % 16)
        return et::fail(ET_ERR_UNSUPPORTED,
                        "interact: the rows of x and dx must be 16-byte aligned");
    if ((uintptr_t)dy % es) return et::fail(ET_ERR_ARG, "interact: dy is not aligned to its type");
    const int64_t dx_b = et::ix_span(batch, ld_dx, width, es);
    if (et::ix_overlap(dx, dx_b, x, et::ix_span(batch, ld_x, width, es)) ||
        et::ix_overlap(dx, dx_b, dy, et::ix_span(batch, ld_dy, copy + np, es)))
        return et::fail(ET_ERR_ARG, "interact: dx overlaps x or dy");
    switch (dtype) {
        case ET_F32:
            et::interact_bwd_launch<float>(x, ld_x, dy, ld_dy, batch, nvec, dim, copy, dx, ld_dx,
                                           flags, stream);
            break;
        case ET_F16:
            et::interact_bwd_launch<_Float16>(x, ld_x, dy, ld_dy, batch, nvec, dim, copy, dx, ld_dx,
                                              flags, stream);
            break;
        default:
            et::interact_bwd_launch<__bf16>(x, ld_x, dy, ld_dy, batch, nvec, dim, copy, dx, ld_dx,
                                            flags, stream);
    }
    ET_LAUNCH_CHECK("k_interact_bwd");
    return ET_OK;
}
