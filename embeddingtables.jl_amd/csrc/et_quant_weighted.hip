// et_quant_weighted.hip — weighted and mean-pooled bags over quantised tables, all five row
// formats (INT8 / INT4, FP8 E4M3 / E5M2, MXFP4): et_quant_weighted_maplookup_prealloc.
// Textually included behind et_mx4.hip: the row layouts, QuantGeom, quant_unpack, quant_slot,
// quant_store, the stripe schedule (quant_vec_grid) and the host validation (quant_validate)
// are et_quant.hip's, the FP8 and MXFP4 decodes are et_fp8.hip's and et_mx4.hip's.  The
// arithmetic is the composition of two contracts of include/embtab.h: v_k is the row's
// dequantised Float32 value under its format's rule, and a bag is acc = w_lo * v_lo, then
// t = w_k * v_k; acc = acc + t in index order, every product and every add rounded once.
//
// One vector kernel, k_qw_vec<DEC, LPR, W>, and one generic kernel, k_qw_generic<DEC, O>.  DEC
// is a decoder policy per format (QwInt<8>, QwInt<4>, QwFp8<E4M3>, QwFp8<E5M2>, QwMx4).  It owns
// where the per-row side data lives (a 4-byte header or a per-block scale byte, fused or split),
// its load, and "16 payload bytes + side data -> F Float32 values, +0 for an out-of-range slot".
//
// Geometry: QuantGeom's.  A lane owns 16 payload bytes and F = 16 or 32 accumulators, LPR lanes
// a bag (masked beyond the row), 64 / LPR bags a wave, 4 waves a workgroup, eight rows of a
// group in flight with tails of 4 / 2 / 1, accumulators that start at -0.0, the static XCD
// stripe schedule.  W = false (unweighted and mean tables) keeps k_quant_vec's register /
// ds_bpermute hand-over of the row indices and has no multiply in the loop; the division of a
// mean table is in the epilogue.
//
// W = true hands (row, weight) to the lane group through LDS.  The row index is already 32 bits
// (idx_row32) and the weight is 32 bits, so a slot is one 8-byte pair.  Each wave owns a private
// slot table of GPW groups x (CH + 1) pairs.  Per chunk every lane writes the K pairs it loaded
// with one 64-bit LDS write each (slot m * LPR + sub of its group), and every row slot is then
// fetched by the whole group with ONE 64-bit LDS read at an immediate offset off the group's
// base register, a broadcast within the group.  The float weighted kernel pays two ds_bpermute
// per slot for the same hand-over, and k_quant_vec a K-way select chain before its
// one.  A wave's LDS operations retire in order, so neither a workgroup barrier nor
// __syncthreads is needed; qw_wave_fence only keeps the compiler from moving the reads over the
// writes (and the next chunk's writes over these reads).  The per-group stride is CH + 1 pairs,
// an odd number of 8-byte words: with a stride of CH = 8 pairs (64 bytes) groups g and g + 2 of
// one read would sit on the same banks at different addresses.
//
// The multiply is never folded into the scale or the bias (that would change the rounding):
// per feature the loop issues the decode, t = w * v, acc + t.  Like the FP8 and MXFP4 kernels
// these opt out of packed Float32 arithmetic (ET_FP8_KERNEL), the INT decoders included: every
// result is pinned bit for bit and the fma, the multiply and the add are issued one feature at
// a time.

namespace et {

struct QwPack {
    et_quant_weighted_desc d[ET_MAX_TABLES_PER_LAUNCH];
};

// Where a lane finds the side data of row r: base + r * stride.
struct QwSide {
    const uint8_t* base;
    uint32_t stride;
};

// The split side data of row r starts at hdr + r * split_stride(dim); the fused side data sits
// behind the row's payload.
template <int BITS_>
struct QwInt {
    static constexpr int BITS = BITS_, F = 128 / BITS_;
    static __device__ __forceinline__ uint32_t split_stride(uint32_t) { return 4u; }
    // blk: the 16-byte vector of the row this lane owns (unused: one header per row)
    static __device__ __forceinline__ QwSide side(const uint8_t* table, const uint8_t* hdr,
                                                  uint32_t ldb, uint32_t payload, uint32_t dim,
                                                  uint32_t blk) {
        return hdr ? QwSide{hdr, 4u} : QwSide{table + payload, ldb};
    }
    static __device__ __forceinline__ uint32_t load_side(const QwSide& s, uint32_t row) {
        return *reinterpret_cast<const uint32_t*>(s.base + (uint64_t)row * s.stride);
    }
    // A zero header makes +0 of every level: fma(q, +0, +0).
    static __device__ __forceinline__ void decode(u32x4 p, uint32_t sd, bool ok, float (&v)[F]) {
        const uint32_t h = ok ? sd : 0u;
        const float s = half_bits_f32(h & 0xffffu), b = half_bits_f32(h >> 16);
        float q[F];
        quant_unpack<BITS>(p, q);
#pragma unroll
        for (int f = 0; f < F; ++f) v[f] = __builtin_fmaf(q[f], s, b);  // exact product
    }
    // Feature f of a row by byte loads (the generic kernel); h: the row's side data.
    static __device__ __forceinline__ float elem(const uint8_t* r, const uint8_t* h, int f,
                                                 bool ok) {
        const float s = ok ? half_bits_f32((uint32_t)h[0] | ((uint32_t)h[1] << 8)) : 0.f;
        const float b = ok ? half_bits_f32((uint32_t)h[2] | ((uint32_t)h[3] << 8)) : 0.f;
        const uint32_t q =
            BITS == 8 ? (uint32_t)r[f] : ((uint32_t)r[f >> 1] >> ((f & 1) * 4)) & 15u;
        return __builtin_fmaf((float)q, s, b);
    }
};

template <int FMT>
struct QwFp8 : QwInt<8> {
    // A NaN or Inf code times a zero scale is NaN: the payload is replaced too (code 0 is +0).
    static __device__ __forceinline__ void decode(u32x4 p, uint32_t sd, bool ok, float (&v)[16]) {
        const uint32_t h = ok ? sd : 0u;
        u32x4 z;
#pragma unroll
        for (int w = 0; w < 4; ++w) z[w] = ok ? p[w] : 0u;
        const float s = half_bits_f32(h & 0xffffu), b = half_bits_f32(h >> 16);
        float q[16];
        fp8_unpack<FMT>(z, q);
#pragma unroll
        for (int f = 0; f < 16; ++f) v[f] = __builtin_fmaf(q[f], s, b);  // exact product
    }
    static __device__ __forceinline__ float elem(const uint8_t* r, const uint8_t* h, int f,
                                                 bool ok) {
        const float s = ok ? half_bits_f32((uint32_t)h[0] | ((uint32_t)h[1] << 8)) : 0.f;
        const float b = ok ? half_bits_f32((uint32_t)h[2] | ((uint32_t)h[3] << 8)) : 0.f;
        const uint32_t code = ok ? (uint32_t)r[f] : 0u;
        return __builtin_fmaf(fp8_decode2<FMT, false>(code)[0], s, b);
    }
};

struct QwMx4 {
    static constexpr int BITS = 4, F = 32;
    static __device__ __forceinline__ uint32_t split_stride(uint32_t dim) {
        return mx4_hdr_stride(dim);
    }
    // A lane's 32 features are one block: its side data is the block's own scale byte.
    static __device__ __forceinline__ QwSide side(const uint8_t* table, const uint8_t* hdr,
                                                  uint32_t ldb, uint32_t payload, uint32_t dim,
                                                  uint32_t blk) {
        return hdr ? QwSide{hdr + blk, mx4_hdr_stride(dim)} : QwSide{table + payload + blk, ldb};
    }
    static __device__ __forceinline__ uint32_t load_side(const QwSide& s, uint32_t row) {
        return s.base[(uint64_t)row * s.stride];
    }
    // A NaN scale byte makes NaN of a zero code: payload and scale byte are both replaced
    // (code 0 under scale byte 0 is +0).
    static __device__ __forceinline__ void decode(u32x4 p, uint32_t sd, bool ok, float (&v)[32]) {
        const float s = mx4_scale_operand(ok ? sd : 0u);
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const uint32_t x = ok ? p[w] : 0u;
            const fp8_f32x2 v0 = ET_MX4_CVT(x, s, 0), v1 = ET_MX4_CVT(x, s, 1);
            const fp8_f32x2 v2 = ET_MX4_CVT(x, s, 2), v3 = ET_MX4_CVT(x, s, 3);
            float* a = v + 8 * w;
            a[0] = v0[0], a[1] = v0[1], a[2] = v1[0], a[3] = v1[1];
            a[4] = v2[0], a[5] = v2[1], a[6] = v3[0], a[7] = v3[1];
        }
    }
    static __device__ __forceinline__ float elem(const uint8_t* r, const uint8_t* h, int f,
                                                 bool ok) {
        const uint32_t byte = ok ? (uint32_t)r[f >> 1] : 0u;
        const float s = mx4_scale_operand(ok ? (uint32_t)h[f >> 5] : 0u);
        const fp8_f32x2 p = ET_MX4_CVT(byte, s, 0);
        return (f & 1) ? p[1] : p[0];
    }
};

// Compiler-only ordering of one wave's LDS writes and reads (no instruction: a wave's LDS
// operations retire in the order they were issued).
__device__ __forceinline__ void qw_wave_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Pairs between the slot tables of two groups: CH slots and one of padding (see the head).
template <int BITS, int LPR>
constexpr int qw_stride() {
    return QuantGeom<BITS, LPR>::CH + 1;
}

// UU rows of one bag (slots i0 .. i0+UU-1 of the group's chunk, all valid): every payload and
// side-data load is issued before the first row is consumed, then the rows are decoded,
// multiplied (W) and added in slot order onto accumulators that start at -0.0.  W: `slots` is
// the group's slot table in LDS, a slot's (row, weight) pair is one 64-bit read; otherwise the
// row comes out of `myr` as in k_quant_vec.
template <typename DEC, int LPR, int UU, bool W>
__device__ __forceinline__ void qw_load_add(
    const char* __restrict__ table, uint32_t ldb, const QwSide& side,
    const uint32_t (&myr)[QuantGeom<DEC::BITS, LPR>::K], int gbase, const uint2* slots, int i0,
    uint32_t voff, float (&acc)[DEC::F], int& bad) {
    using G = QuantGeom<DEC::BITS, LPR>;
    constexpr int F = DEC::F;
    u32x4 buf[UU];
    uint32_t sd[UU];
    float w[UU];
    bool ok[UU];
#pragma unroll
    for (int u = 0; u < UU; ++u) {
        uint32_t r;
        if constexpr (W) {
            const uint2 pr = slots[i0 + u];
            r = pr.x;
            w[u] = __builtin_bit_cast(float, pr.y);
        } else {
            r = quant_slot<LPR, G::K>(myr, gbase, i0 + u);
        }
        ok[u] = r != ~0u;
        const uint32_t row = ok[u] ? r : 0u;
        buf[u] = *reinterpret_cast<const u32x4*>(table + (uint64_t)row * ldb + voff);
        sd[u] = DEC::load_side(side, row);
    }
#pragma unroll
    for (int u = 0; u < UU; ++u) {
        bad += ok[u] ? 0 : 1;
        float v[F];
        DEC::decode(buf[u], sd[u], ok[u], v);
#pragma unroll
        for (int f = 0; f < F; ++f) {
            if constexpr (W) {
                const float t = w[u] * v[f];  // an out-of-range row is +0, still multiplied
                acc[f] = acc[f] + t;
            } else {
                acc[f] = acc[f] + v[f];
            }
        }
    }
}

// Vector kernel: grid = kXcds * ntables * stripe_chunks workgroups of 256; a workgroup owns
// 4 * GPW consecutive bags of one table.  `out` is the destination's ET_* element type.  W: every
// table of the launch carries weights (sum mode); otherwise none does and each table's own mode
// says sum or mean.
template <typename DEC, int LPR, bool W>
__global__ ET_FP8_KERNEL __launch_bounds__(256) void k_qw_vec(
    QwPack pack, QuantStripes sm, int ntables, int64_t batch, void* __restrict__ dst,
    int64_t ld_dst, int out, int nt, int64_t stripe_chunks, int64_t nchunks) {
    using G = QuantGeom<DEC::BITS, LPR>;
    constexpr int F = DEC::F, CH = G::CH, K = G::K, U = G::U, GPW = G::GPW;
    constexpr int STRIDE = qw_stride<DEC::BITS, LPR>();
    static_assert(G::F == F, "a lane owns 16 payload bytes");
    __shared__ uint2 s_slots[W ? 4 * GPW * STRIDE : 1];
    const int x = blockIdx.x % kXcds;
    const int64_t slot = blockIdx.x / kXcds;
    const uint32_t e = sm.e[x][slot % ntables];
    const int64_t j = slot / ntables;
    const int64_t chunk = (int64_t)(e >> 5) * stripe_chunks + j;
    if (j >= stripe_chunks || chunk >= nchunks) return;
    const et_quant_weighted_desc& d = pack.d[e & 31u];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = lane / LPR, sub = lane % LPR, gbase = g * LPR;
    const int64_t bag = chunk * (4 * GPW) + wave * GPW + g;
    if (bag >= batch) return;

    const char* table = reinterpret_cast<const char*>(d.table);
    const uint32_t ldb = (uint32_t)d.ld_bytes, nr = (uint32_t)d.nrows;
    const uint32_t payload = (uint32_t)d.dim * DEC::BITS / 8u;
    const int vpr = (int)(payload / 16u);
    const uint32_t blk = (uint32_t)(sub < vpr ? sub : vpr - 1);
    const uint32_t voff = 16u * blk;
    const QwSide side = DEC::side(reinterpret_cast<const uint8_t*>(d.table),
                                  reinterpret_cast<const uint8_t*>(d.hdr), ldb, payload,
                                  (uint32_t)d.dim, blk);
    int64_t lo, hi;
    int bad;
    ragged_range(d.colptr, bag, d.nnz, lo, hi, bad);
    const int64_t* __restrict__ ip = d.idx + lo;
    const float* __restrict__ wp = W ? d.weights + lo : nullptr;
    const int64_t len = hi - lo;
    uint2* slots = s_slots + (W ? (wave * GPW + g) * STRIDE : 0);  // this group's slot table

    float acc[F];
#pragma unroll
    for (int f = 0; f < F; ++f) acc[f] = -0.f;

    for (int64_t c0 = 0; c0 < len; c0 += CH) {
        const int cnt = len - c0 < CH ? (int)(len - c0) : CH;
        uint32_t myr[K];  // lanes past the end re-read the chunk's last slot, weight included
#pragma unroll
        for (int m = 0; m < K; ++m) {
            const int i = m * LPR + sub;
            const int64_t k = c0 + (i < cnt ? i : cnt - 1);
            myr[m] = idx_row32((long long)ip[k], nr);
            if constexpr (W) slots[i] = make_uint2(myr[m], __builtin_bit_cast(uint32_t, wp[k]));
        }
        if constexpr (W) qw_wave_fence();
#define ET_QW_LOAD_ADD(UU, I0)                                                                 \
    qw_load_add<DEC, LPR, UU, W>(table, ldb, side, myr, gbase, slots, I0, voff, acc, bad)
        int i0 = 0;
        if constexpr (K > 1) {
            // CH == U: a full chunk is one batch at compile-time slots
            if (cnt == CH) {
                ET_QW_LOAD_ADD(U, 0);
                i0 = CH;
            }
        } else {
            for (; i0 + U <= cnt; i0 += U) ET_QW_LOAD_ADD(U, i0);
        }
        if (cnt - i0 >= 4) {
            ET_QW_LOAD_ADD(4, i0);
            i0 += 4;
        }
        if (cnt - i0 >= 2) {
            ET_QW_LOAD_ADD(2, i0);
            i0 += 2;
        }
        if (cnt - i0 >= 1) ET_QW_LOAD_ADD(1, i0);
#undef ET_QW_LOAD_ADD
        if constexpr (W) qw_wave_fence();  // the next chunk's writes stay behind these reads
    }
    if (bad && sub == 0) note_oob(bad);
    if (sub >= vpr) return;
    if (len <= 0) {  // an empty bag is +0
#pragma unroll
        for (int f = 0; f < F; ++f) acc[f] = 0.f;
    } else if (!W && d.mode == ET_POOL_MEAN) {
        const float flen = (float)len;
#pragma unroll
        for (int f = 0; f < F; ++f) acc[f] = acc[f] / flen;
    }
    const int64_t o = bag * ld_dst + d.dst_row_off + (int64_t)sub * F;
    if (out == ET_F32) {
        float* p = reinterpret_cast<float*>(dst) + o;
        quant_store<float, F>(p, acc, quant_aligned16(p), nt);
        return;
    }
    // One rounding from the Float32 result to 16 bits: opaque, so that O(w * v) of a one-entry
    // bag (or O(acc / len)) never folds into a mixed-precision instruction that rounds the exact
    // result once (k_weighted_vec's and sgd_apply_t's barrier).
#pragma unroll
    for (int f = 0; f < F; ++f) asm volatile("" : "+v"(acc[f]));
    if (out == ET_F16) {
        _Float16* p = reinterpret_cast<_Float16*>(dst) + o;
        quant_store<_Float16, F>(p, acc, quant_aligned16(p), nt);
    } else {
        __bf16* p = reinterpret_cast<__bf16*>(dst) + o;
        quant_store<__bf16, F>(p, acc, quant_aligned16(p), nt);
    }
}

// Generic kernel: any dim, alignment and leading dimension (byte reads only).  One wave per bag,
// lanes stride over the features, the bag's entries sequential per feature.  An entry's weight
// is a wave-uniform load; a table's weights (or none) and its mode are read from its descriptor.
template <typename DEC, typename O>
__global__ ET_FP8_KERNEL __launch_bounds__(256) void k_qw_generic(
    QwPack pack, int ntables, int64_t batch, O* __restrict__ dst, int64_t ld_dst, int nt) {
    constexpr int K = 4;
    const int64_t item = blockIdx.x;
    const et_quant_weighted_desc& d = pack.d[(int)(item % ntables)];
    const int64_t chunk = item / ntables;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t bag = chunk * 4 + wave;
    if (bag >= batch) return;
    int64_t lo, hi;
    int clamped;
    ragged_range(d.colptr, bag, d.nnz, lo, hi, clamped);
    if (clamped && lane == 0) note_oob(clamped);
    const uint8_t* table = reinterpret_cast<const uint8_t*>(d.table);
    const uint8_t* hdr = reinterpret_cast<const uint8_t*>(d.hdr);
    const int dim = d.dim;
    const int64_t payload = (int64_t)dim * DEC::BITS / 8;
    const uint32_t sstride = DEC::split_stride((uint32_t)dim);
    const float* __restrict__ wp = d.weights;
    const bool mean = !wp && d.mode == ET_POOL_MEAN && hi > lo;
    const float flen = (float)(hi - lo);
    O* out = dst + bag * ld_dst + d.dst_row_off;
    for (int f0 = 0; f0 < dim; f0 += 64 * K) {
        float acc[K];
#pragma unroll
        for (int k = 0; k < K; ++k) acc[k] = 0.f;
        for (int64_t i = lo; i < hi; ++i) {
            uint64_t row = (uint64_t)(d.idx[i] - 1);
            const bool ok = row < (uint64_t)d.nrows;
            if (!ok && lane == 0 && f0 == 0) note_oob();
            row = ok ? row : 0;
            const uint8_t* r = table + row * (uint64_t)d.ld_bytes;
            const uint8_t* h = hdr ? hdr + row * sstride : r + payload;
            const float w = wp ? wp[i] : 1.f;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const int f = f0 + lane + 64 * k;
                if (f < dim) {
                    float v = DEC::elem(r, h, f, ok);
                    if (wp) v = w * v;  // an out-of-range row is +0, still multiplied
                    acc[k] = i == lo ? v : acc[k] + v;
                }
            }
        }
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int f = f0 + lane + 64 * k;
            if (f < dim) {
                float y = mean ? acc[k] / flen : acc[k];
                if constexpr (sizeof(O) == 2) asm volatile("" : "+v"(y));  // one rounding to O
                if (nt)
                    store_scalar<true>(out + f, O(y));
                else
                    store_scalar<false>(out + f, O(y));
            }
        }
    }
}

// ---------------------------------------------------------------------------
// Host dispatch
// ---------------------------------------------------------------------------

// The descriptor as the ragged et_quant_desc the per-format rules (quant_validate) and the
// stripe placement (quant_vec_grid) read.
inline et_quant_desc qw_as_quant(const et_quant_weighted_desc& d) {
    et_quant_desc q;
    q.table = d.table;
    q.ld_bytes = d.ld_bytes;
    q.nrows = d.nrows;
    q.dim = d.dim;
    q.bits = d.bits;
    q.hdr = d.hdr;
    q.pool = 0;
    q.reserved = 0;
    q.idx = d.idx;
    q.ld_idx = 0;
    q.colptr = d.colptr;
    q.nnz = d.nnz;
    q.dst_row_off = d.dst_row_off;
    return q;
}

template <typename DEC, int LPR>
int launch_qw_vec(bool w, const QwPack& pack, int n, int64_t batch, void* dst, int64_t ld_dst,
                  int out, bool nt, hipStream_t s) {
    QuantPack qp;
    for (int t = 0; t < n; ++t) qp.d[t] = qw_as_quant(pack.d[t]);
    QuantGrid g;
    const int rc = quant_vec_grid(qp, n, batch, 4 * QuantGeom<DEC::BITS, LPR>::GPW, &g);
    if (rc != ET_OK) return rc;
    if (w)
        hipLaunchKernelGGL((k_qw_vec<DEC, LPR, true>), dim3((unsigned)g.grid), dim3(256), 0, s,
                           pack, g.sm, n, batch, dst, ld_dst, out, nt ? 1 : 0, g.stripe_chunks,
                           g.nchunks);
    else
        hipLaunchKernelGGL((k_qw_vec<DEC, LPR, false>), dim3((unsigned)g.grid), dim3(256), 0, s,
                           pack, g.sm, n, batch, dst, ld_dst, out, nt ? 1 : 0, g.stripe_chunks,
                           g.nchunks);
    ET_LAUNCH_CHECK("k_qw_vec");
    return ET_OK;
}

template <typename DEC, typename O>
int launch_qw_generic_o(const QwPack& pack, int n, int64_t batch, void* dst, int64_t ld_dst,
                        bool nt, hipStream_t s) {
    const int64_t grid = (batch + 3) / 4 * n;
    if (grid > 0x7fffffffll) return fail(ET_ERR_ARG, "grid too large");
    hipLaunchKernelGGL((k_qw_generic<DEC, O>), dim3((unsigned)grid), dim3(256), 0, s, pack, n,
                       batch, reinterpret_cast<O*>(dst), ld_dst, nt ? 1 : 0);
    ET_LAUNCH_CHECK("k_qw_generic");
    return ET_OK;
}

// One group of tables: lpr == 0 the generic kernel, else the vector kernel of that lane group.
template <typename DEC>
int launch_qw(int lpr, bool w, const QwPack& pack, int n, int64_t batch, void* dst,
              int64_t ld_dst, int out, bool nt, hipStream_t s) {
    switch (lpr) {
        case 0:
            return out == ET_F32   ? launch_qw_generic_o<DEC, float>(pack, n, batch, dst, ld_dst, nt, s)
                   : out == ET_F16 ? launch_qw_generic_o<DEC, _Float16>(pack, n, batch, dst, ld_dst, nt, s)
                                   : launch_qw_generic_o<DEC, __bf16>(pack, n, batch, dst, ld_dst, nt, s);
        case 1: return launch_qw_vec<DEC, 1>(w, pack, n, batch, dst, ld_dst, out, nt, s);
        case 2: return launch_qw_vec<DEC, 2>(w, pack, n, batch, dst, ld_dst, out, nt, s);
        case 4: return launch_qw_vec<DEC, 4>(w, pack, n, batch, dst, ld_dst, out, nt, s);
        case 8: return launch_qw_vec<DEC, 8>(w, pack, n, batch, dst, ld_dst, out, nt, s);
        case 16: return launch_qw_vec<DEC, 16>(w, pack, n, batch, dst, ld_dst, out, nt, s);
        case 32: return launch_qw_vec<DEC, 32>(w, pack, n, batch, dst, ld_dst, out, nt, s);
        case 64: return launch_qw_vec<DEC, 64>(w, pack, n, batch, dst, ld_dst, out, nt, s);
    }
    return fail(ET_ERR_UNSUPPORTED, "quantised weighted lane group %d", lpr);
}

// Validate everything (the format's own rules through quant_validate on the converted
// descriptors, then what the weighted form adds), group the tables by (kernel key, weights or
// none) and launch one kernel per group.
inline int qw_dispatch(int out, int format, const et_quant_weighted_desc* descs, int ntables,
                       int64_t batch, void* dst, int64_t ld_dst, uint32_t flags, hipStream_t s) {
    if (format != ET_QUANT_INT && format != ET_FP8_E4M3 && format != ET_FP8_E5M2 &&
        format != ET_QUANT_MXFP4)
        return fail(ET_ERR_UNSUPPORTED, "format %d is none of 0 (INT8 / INT4), 1 (E4M3), 2 (E5M2), "
                    "3 (MXFP4)", format);
    et_quant_desc conv[ET_MAX_TABLES_PER_LAUNCH];
    const bool readable = descs && ntables > 0 && ntables <= ET_MAX_TABLES_PER_LAUNCH;
    for (int t = 0; readable && t < ntables; ++t) conv[t] = qw_as_quant(descs[t]);
    int key_of[ET_MAX_TABLES_PER_LAUNCH];
    bool work;
    const bool mx4 = format == ET_QUANT_MXFP4;
    const int only_bits = format == ET_QUANT_INT ? 0 : mx4 ? 4 : 8;
    const int rc = quant_validate(out, descs ? conv : nullptr, ntables, batch, dst, ld_dst, flags,
                                  only_bits, key_of, &work, mx4);
    if (rc != ET_OK || !work) return rc;
    for (int t = 0; t < ntables; ++t) {
        const et_quant_weighted_desc& d = descs[t];
        if (!d.colptr) return fail(ET_ERR_ARG, "table %d: NULL colptr (bags are always ragged)", t);
        if (d.mode != ET_POOL_SUM && d.mode != ET_POOL_MEAN)
            return fail(ET_ERR_ARG, "table %d: mode %d", t, d.mode);
        if (d.mode == ET_POOL_MEAN && d.weights)
            return fail(ET_ERR_UNSUPPORTED, "table %d: weights with mean pooling", t);
        if (reinterpret_cast<uintptr_t>(d.weights) & 3u)
            return fail(ET_ERR_ARG, "table %d: weights not 4-byte aligned", t);
        // quant_validate's key is bits * 256 + lane group, 0 for a generic table of either
        // width: the generic kernel here has its width at compile time
        if (format == ET_QUANT_INT && key_of[t] == 0) key_of[t] = d.bits * 256;
    }
    open_side_streams(s);
    const bool nt = (flags & ET_FLAG_NONTEMPORAL) != 0;
    bool done[ET_MAX_TABLES_PER_LAUNCH] = {false};
    for (int t0 = 0; t0 < ntables; ++t0) {
        if (done[t0] || key_of[t0] < 0) continue;
        const bool w = descs[t0].weights != nullptr;
        QwPack pack;
        int n = 0;
        for (int t = t0; t < ntables; ++t) {
            if (done[t] || key_of[t] != key_of[t0] || (descs[t].weights != nullptr) != w) continue;
            pack.d[n++] = descs[t];
            done[t] = true;
        }
        const int key = key_of[t0], lpr = key % 256;
        int r;
        if (format == ET_FP8_E4M3)
            r = launch_qw<QwFp8<ET_FP8_E4M3>>(lpr, w, pack, n, batch, dst, ld_dst, out, nt, s);
        else if (format == ET_FP8_E5M2)
            r = launch_qw<QwFp8<ET_FP8_E5M2>>(lpr, w, pack, n, batch, dst, ld_dst, out, nt, s);
        else if (mx4)
            r = launch_qw<QwMx4>(lpr, w, pack, n, batch, dst, ld_dst, out, nt, s);
        else if (key / 256 == 8)
            r = launch_qw<QwInt<8>>(lpr, w, pack, n, batch, dst, ld_dst, out, nt, s);
        else
            r = launch_qw<QwInt<4>>(lpr, w, pack, n, batch, dst, ld_dst, out, nt, s);
        if (r != ET_OK) return r;
    }
    return ET_OK;
}

}  // namespace et

extern "C" int et_quant_weighted_maplookup_prealloc(int dst_dtype, int format,
                                                    const et_quant_weighted_desc* descs,
                                                    int32_t ntables, int64_t batch, void* dst,
                                                    int64_t ld_dst, uint32_t flags, void* stream) {
    et::clear_err();
    return et::qw_dispatch(dst_dtype, format, descs, ntables, batch, dst, ld_dst, flags,
                           static_cast<hipStream_t>(stream));
}
