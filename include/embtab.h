/*
 * embtab.h — C ABI of libembtab_hip.so, the MI355X (gfx950) embedding-table engine.
 *
 * This is the drop-in boundary for the hot path of darchr/EmbeddingTables.jl:
 * the Julia package's `lookup!`, `maplookup!(::PreallocationStrategy, …)` and
 * `update!(::Descent, …)` methods are re-targeted (by a thin `ccall` layer, see
 * INTEGRATION.md) onto the entry points below.  Every entry point:
 *
 *   - takes plain pointers and sizes only (no torch / no Julia types);
 *   - takes DEVICE pointers for every array argument, except arrays of
 *     descriptors (`et_lookup_desc*`, `et_update_desc*`), which live in HOST
 *     memory and are copied into the kernel argument segment at launch;
 *   - is stream-ordered on the caller's `hipStream_t` (passed as `void*`;
 *     NULL = the legacy default stream) and never synchronises the device,
 *     allocates or frees memory, so it may be captured into a hipGraph;
 *   - returns an `int` status (ET_OK = 0, negative = error).  The message for
 *     the last error of the calling thread is `et_last_error()`.
 *
 * Memory layout (identical to the reference, column-major Julia arrays):
 *   - a table is a D x R matrix whose column `r` (1-based) — one embedding
 *     vector of D contiguous elements — starts at `table + (r-1)*ld_table`
 *     (reference `columnpointer`, src/simple.jl:52-55, src/EmbeddingTables.jl:83-85);
 *   - index arrays are Int64 and 1-BASED, as in Julia; a P x B index matrix
 *     (pool P, batch B) stores bag j's P entries at `idx + j*ld_idx`;
 *   - outputs / gradients are D x B column-major with leading dimension `ld`.
 *   - all leading dimensions are in ELEMENTS, not bytes.
 *
 * Out-of-range indices are undefined behaviour in the reference
 * (`@inbounds`, src/lookup.jl).  Here they never fault the GPU: a bad index
 * contributes a zero row (lookup) or is skipped (update), and is counted in a
 * device-side error word readable with `et_check_errors`.
 *
 * Special values.  Every sum, product and conversion below is the IEEE-754 operation of
 * its type in round-to-nearest-even, with nothing flushed: subnormal inputs, sums and
 * results are kept.  Signed zeros and +-Inf are bit-identical to the reference's CPU
 * algorithms (a pooled sum starts with a copy of its first row, so a bag of -0 rows is
 * -0; an empty bag and an update's column sum start from +0), and Inf stays Inf where the
 * reference's adds keep it: Inf + x is never turned into NaN.  NaN is guaranteed by
 * position, not by sign or payload (a generated NaN differs between platforms), except in
 * pure copies: a vector-index gather, and a one-entry bag of a type that is its own
 * accumulator, return the stored bits.  The zero row an out-of-range index contributes is
 * a select, never a product: it is +0 whatever the table holds, NaN and Inf included.
 * Where a definition multiplies (weights, row-wise scales), 0 * Inf and 0 * NaN are NaN
 * as IEEE-754 has them.  Integer sums wrap.
 */
#ifndef EMBTAB_H
#define EMBTAB_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ET_ABI_VERSION 9

/* Status codes. */
#define ET_OK 0
#define ET_ERR_ARG (-1)         /* invalid argument (message in et_last_error) */
#define ET_ERR_HIP (-2)         /* a HIP runtime call failed */
#define ET_ERR_WORKSPACE (-3)   /* workspace missing or too small */
#define ET_ERR_UNSUPPORTED (-4) /* dtype / mode not implemented */

/* Element types of tables, outputs and gradients. */
#define ET_F32 0
#define ET_F16 1
#define ET_F64 2
#define ET_I32 3
#define ET_I64 4
#define ET_BF16 5 /* bfloat16 tables: pooled sums accumulate in fp32 and round once (RNE);
                     not a reference type (Julia's reference never uses BFloat16) */

/* Flags (bitwise OR). */
#define ET_FLAG_NONTEMPORAL 1u   /* non-temporal stores of outputs / updated rows
                                    (reference Val{Nontemporal}, src/sparseupdate.jl:165) */
#define ET_FLAG_F16_FP32_ACC 2u  /* F16 pooled sums (and F16 SGD sums) accumulate in fp32
                                    and round once; default F16 mode rounds to fp16 after
                                    every add like Julia Float16 arithmetic */
#define ET_FLAG_EXACT_UPDATE 4u  /* sparse SGD: never split a hot row's occurrence list, so
                                    every row's gradient is summed serially in occurrence
                                    order (bit-identical to the reference, slower on skew) */
#define ET_FLAG_SGD_UNFUSED 8u   /* sparse SGD: w - eta*acc with two roundings, the
                                    reference's generic path (src/sparseupdate.jl:57-95);
                                    default is fma(-eta, acc, w), its specialized path
                                    (src/sparseupdate.jl:97-129) */
#define ET_FLAG_SGD_F64_ALPHA 16u /* with ET_FLAG_SGD_UNFUSED: evaluate w - eta*acc in
                                    Float64, as the multi-table generic path does with the
                                    unconverted opt.eta (src/sparseupdate.jl:232) */
#define ET_FLAG_SGD_INDEX_ONLY 32u /* sparse SGD, phase 1 of 2: only the index work (keys,
                                    sort, segments, chunk records) into the workspace; reads
                                    idx, never delta or the tables (delta may be NULL) — the
                                    reference's "index all" phase, src/sparseupdate.jl:210-213 */
#define ET_FLAG_SGD_APPLY_ONLY 64u /* sparse SGD, phase 2 of 2: the gradient sums and row
                                    updates from a workspace that an INDEX_ONLY call with the
                                    same descriptors, flags and workspace filled earlier in
                                    stream order ("update all", :216-237); idx is not read
                                    again, so it may be refilled once phase 1 is done */
#define ET_FLAG_SGD_HOT_PASS 128u /* sparse SGD, non-exact Float32 dim-128 tables with pool
                                    <= 32: the longest occurrence lists (up to 120 columns
                                    per table, by a log2 length threshold) are summed
                                    bag-major over 1024-bag windows instead of by per-
                                    occurrence gathers (deterministic; EXPERIMENTAL, slower
                                    today — DESIGN.md §7) */
#define ET_FLAG_EXACT_IF_FAST 256u /* sparse SGD, the bindings' default: since ABI v9 the
                                    same as ET_FLAG_EXACT_UPDATE — the exact mode's serial-
                                    chain path covers every element type and gradient size
                                    up to a batch of 2^27 - 1 bags (ABI v8 resolved it to the
                                    split mode for non-Float32 tables and for batch *
                                    ld_delta >= 2^30).  A batch of 2^27 bags or more is still
                                    exact but sums every column in one chunk (one wave per
                                    column: slow for hot columns) */

/* Occurrences per chunk of the non-exact sparse SGD: a column with more occurrences than
 * this is summed as ordered partial sums of ET_SGD_CHUNK consecutive occurrences (so a
 * column with at most ET_SGD_CHUNK occurrences is always the serial, bit-identical sum).
 * 256 measured 2% faster than 512 and 7% faster than 1024 on BASELINE config 4. */
#define ET_SGD_CHUNK 256

/* Tables per launch carried in the kernel-argument segment; longer lists are
 * split into several launches by the library. */
#define ET_MAX_TABLES_PER_LAUNCH 32

/* ABI version compiled into the library (== ET_ABI_VERSION). */
int et_abi_version(void);

/* Message of the last failed call on this thread ("" if none). */
const char* et_last_error(void);

/* Non-reducing gather: dst[:, j] = table[:, idx[j]] for j in 0..n-1
 * (bit copy for every dtype).
 * Replaces lookup!(dst, A, I::AbstractVector) — reference src/lookup.jl:51-67
 * (lookup_generic!), :70-87 (lookup_static! SVector) and dispatch :90-102. */
int et_gather(int dtype, const void* table, int64_t ld_table, int64_t nrows, int32_t dim,
              const int64_t* idx, int64_t n, void* dst, int64_t ld_dst, uint32_t flags,
              void* stream);

/* Reducing (pooled-sum) lookup: dst[:, j] = sum_{i=0..pool-1} table[:, idx[j*ld_idx + i]],
 * accumulated sequentially in pool order starting from the first row (pool == 0
 * writes zeros).
 * Replaces lookup!(dst, A, I::AbstractMatrix) — reference src/lookup.jl:108-132
 * (lookup_generic!), :134-165 (lookup_static_inner / lookup_static! TiledSIMD) and
 * dispatch :167-182. */
int et_pooled_sum(int dtype, const void* table, int64_t ld_table, int64_t nrows, int32_t dim,
                  const int64_t* idx, int32_t pool, int64_t ld_idx, int64_t batch, void* dst,
                  int64_t ld_dst, uint32_t flags, void* stream);

/* One table of a fused multi-table lookup. */
typedef struct et_lookup_desc {
    const void* table;   /* device pointer to column 1 of the table */
    int64_t ld_table;    /* elements between consecutive columns (>= dim) */
    int64_t nrows;       /* number of columns R (embeddings) in the table */
    int32_t dim;         /* feature size D */
    int32_t pool;        /* P: indices per bag; 1 for a vector (non-reducing) index */
    const int64_t* idx;  /* device pointer, 1-based Int64, bag j at idx + j*ld_idx */
    int64_t ld_idx;      /* elements between consecutive bags' index lists */
    int64_t dst_row_off; /* first row of this table's block in dst (prependrows + sum of
                            previous tables' dims) */
    int64_t cols_per_page; /* 0: contiguous table.  > 0: a PAGED table (the reference's
                            SplitEmbedding, src/split.jl:3-86): `table` is a device array of
                            page pointers, column r (1-based) lives in page (r-1)/cols_per_page
                            at column (r-1)%cols_per_page, ld_table apart within a page;
                            every page pointer must be 16-byte aligned (hipMalloc gives 256)
                            when ld_table * elsize is a multiple of 16 bytes; otherwise the
                            generic (element-aligned) kernels run.  cols_per_page = 1 is a
                            COLUMN-POINTER table — `table` holds one pointer per column, any
                            layout — the form any `columnpointer`-only table type takes
                            (README.md:288-307); ld_table is then only that alignment switch */
} et_lookup_desc;

/* Fused lookup + concat (PreallocationStrategy):
 * dst[desc[t].dst_row_off + (0:dim_t-1), j] = lookup(table_t, idx_t)[:, j] for every
 * table t and bag j, written in place into the (ld_dst x batch) destination.
 * Rows of dst not covered by any table (the prepended rows) are not touched.
 * `descs` is a HOST array of `ntables` descriptors.
 * Replaces maplookup!(::PreallocationStrategy, dst, tables, I) — reference
 * src/lookup.jl:316-371 (and maplookup :305-314 once dst is allocated). */
int et_maplookup_prealloc(int dtype, const et_lookup_desc* descs, int32_t ntables,
                          int64_t batch, void* dst, int64_t ld_dst, uint32_t flags,
                          void* stream);

/* et_maplookup_prealloc with a caller-owned QUEUE BLOCK (ABI v9): `queue` is
 * ET_LOOKUP_QUEUE_BYTES of 16-byte aligned device memory, ZERO before its first use; the
 * multi-table launch then takes its work items from per-XCD queues in that block (an XCD
 * that finishes its own items takes over another's, ~1% faster on BASELINE config 3) and
 * leaves the block zero again when it completes.  A block may serve any number of calls
 * that are ordered with each other (one stream, a captured and replayed HIP graph), never
 * two calls that may run at the same time.  queue == NULL is et_maplookup_prealloc (the
 * static XCD stripe schedule).  Results are identical either way. */
#define ET_LOOKUP_QUEUE_BYTES 128
int et_maplookup_prealloc_q(int dtype, const et_lookup_desc* descs, int32_t ntables,
                            int64_t batch, void* dst, int64_t ld_dst, uint32_t flags, void* queue,
                            void* stream);

/* PreallocationStrategy{U} with a destination of another floating type than the
 * tables (src/lookup.jl:284-315: `similar(example(x), U, ...)`): every pooled sum is
 * formed in the table type (dtype; ET_FLAG_F16_FP32_ACC as for et_pooled_sum), then
 * converted to dst_dtype on the store.  Float types only (ET_F32/F64/F16/BF16);
 * dst_dtype == dtype is et_maplookup_prealloc. */
int et_maplookup_prealloc_to(int dtype, int dst_dtype, const et_lookup_desc* descs,
                             int32_t ntables, int64_t batch, void* dst, int64_t ld_dst,
                             uint32_t flags, void* stream);

/* One table of a (multi-table) fused sparse-SGD update. */
typedef struct et_update_desc {
    void* table;         /* device pointer, updated in place */
    int64_t ld_table;
    int64_t nrows;
    int32_t dim;
    int32_t pool;        /* indices per bag (1 for a vector index) */
    const void* delta;   /* gradient wrt the lookup output: dim x batch, column j at
                            delta + j*ld_delta (may be a row block of a Preallocation
                            gradient, ld_delta = prependrows + sum(dims)) */
    int64_t ld_delta;
    const int64_t* idx;  /* the indices of the forward lookup (1-based) */
    int64_t ld_idx;
    int64_t batch;
    int64_t cols_per_page; /* 0 or a paged table, as in et_lookup_desc */
} et_update_desc;

/* Bytes of device workspace needed by et_sparse_sgd for these descriptors (any
 * alignment: the library lays its buffers out from the workspace's first 256-byte
 * boundary; the size includes that slack). */
int et_sgd_workspace_size(const et_update_desc* descs, int32_t ntables, int64_t* bytes);

/* Fused sparse SGD (Flux.Descent) over one or many tables:
 *   for every table t and every distinct column r referenced by idx_t:
 *     acc = +0 ; for each occurrence (in occurrence order) of r, in bag j: acc += delta_t[:, j]
 *     table_t[:, r] = muladd(-eta, acc, table_t[:, r])   (default: fused, Float32(eta))
 *                   = table_t[:, r] - eta*acc            (ET_FLAG_SGD_UNFUSED)
 * dtype ET_F32 (the reference's tested type; vector kernels), ET_F64, ET_F16 and
 * ET_BF16 (generic kernels): the table and delta share the element type T, eta is
 * convert(T, eta); Float64 accumulates in double, Float16 in Julia Float16 arithmetic
 * (every op rounded to half) or in fp32 with ET_FLAG_F16_FP32_ACC, BFloat16 in fp32;
 * the fused muladd of 16-bit types is one fp32 fma rounded to T (oracle/embtab_oracle.c
 * states the exact model).  Without ET_FLAG_EXACT_UPDATE, occurrence lists
 * longer than the library's chunk length are summed as per-chunk partial sums
 * combined in chunk order (deterministic, not bit-identical to the serial sum).
 * Replaces update!(::Descent, table, ::SparseEmbeddingUpdate, indexer, Val(NT)) —
 * reference src/sparseupdate.jl:160-178 with index! (src/utils.jl:306-314) and
 * _update_specialized_impl! / _update_generic_impl! (:57-154); for ntables > 1 the
 * multi-table update!(opt, tables, grads, indexers; num_splits) :199-238. */
int et_sparse_sgd(int dtype, const et_update_desc* descs, int32_t ntables, double eta,
                  uint32_t flags, void* workspace, int64_t ws_bytes, void* stream);

/* et_sparse_sgd that also copies every table's indices as its index phase reads them (ABI
 * v8): snaps is a HOST array of ntables (<= ET_MAX_TABLES_PER_LAUNCH) device pointers;
 * snaps[t] != NULL receives table t's pool x batch Int64 indices, contiguous (bag-major),
 * stream-ordered inside the index phase (not written by an APPLY_ONLY call).  The copy the
 * multi-table update!(opt, tables, grads, indexers) keeps for filling indexers[i]
 * (src/sparseupdate.jl:210-213) when the caller may refill the index buffers before reading
 * them: 8 bytes written per occurrence beside the keys instead of a separate read-and-write
 * pass.  16-byte aligned snapshots keep the vectorized key pass. */
int et_sparse_sgd_snap(int dtype, const et_update_desc* descs, int32_t ntables, double eta,
                       uint32_t flags, int64_t* const* snaps, void* workspace, int64_t ws_bytes,
                       void* stream);

/* Update from a prebuilt Indexer (et_index_build layout) over its cumulative entries
 * [ubegin, uend) — the reference's lower-level
 * update!(table, ::SparseEmbeddingUpdate, indexer::AbstractIndexer, alpha, Val(NT)),
 * src/sparseupdate.jl:46-154, where an IndexerView (src/utils.jl:320-338) selects a
 * range of distinct columns.  Every column's gradient is summed serially in `map`
 * order (exact).  `cumulative_*` and `map` are device arrays as written by
 * et_index_build; `eta` is the value the reference passes as `alpha`;
 * `cols_per_page` as in et_lookup_desc (0 = contiguous). */
int et_update_indexed(int dtype, void* table, int64_t ld_table, int64_t cols_per_page,
                      int64_t nrows, int32_t dim, const void* delta, int64_t ld_delta, const int64_t* cumulative_col,
                      const int64_t* cumulative_off, int64_t ubegin, int64_t uend,
                      const int64_t* map, double eta, uint32_t flags, void* stream);

/* Bytes of device workspace needed by et_index_build for n occurrences. */
int et_index_workspace_size(int64_t n, int64_t* bytes);

/* The reference's Indexer on the device: groups the occurrences of a P x B (or
 * vector, pool = 1) index array by column, with the distinct columns in
 * FIRST-SEEN order and each column's occurrences in occurrence order.
 * Outputs (device, int64, 1-based like the reference):
 *   cumulative_col[u], cumulative_off[u] for u < U, and the terminator
 *   cumulative_col[U] = 0, cumulative_off[U] = n + 1;
 *   map[k] = gradient column (bag, 1-based) of the k-th grouped occurrence;
 *   *nunique_dev = U.
 * Arrays must hold n+1 (cumulative) and n (map) entries.
 * Replaces index!(::Indexer, A, maxindex) — reference src/utils.jl:306-314 with
 * histogram! :131-167, prefixsum! :170-239, remap! :242-272. */
int et_index_build(const int64_t* idx, int32_t pool, int64_t ld_idx, int64_t batch,
                   int64_t nrows, int64_t* cumulative_col, int64_t* cumulative_off,
                   int64_t* map, int64_t* nunique_dev, void* workspace, int64_t ws_bytes,
                   void* stream);

/* ---------------------------------------------------------------------------------
 * Variable-length (ragged) bags.  The reference has no ragged form: its pooled lookup
 * takes a dense P x B index matrix.  These entries extend its pooled sum
 * (src/lookup.jl:134-147) and its per-column serial gradient sum
 * (src/sparseupdate.jl:97-129) to bags of any length, given as the pattern of a Julia
 * SparseMatrixCSC: `idx` is rowval (the indices of all bags, back to back) and `colptr`
 * has batch + 1 entries, Int64 and 1-BASED, non-decreasing; bag j (0-based) owns
 * idx[colptr[j]-1 .. colptr[j+1]-2].
 *
 * `nnz` is the CAPACITY of idx, not the number of entries in use: the kernels find a bag
 * from colptr alone and use nnz only to clamp, so idx and colptr may be refilled in place
 * (also under a captured HIP graph) with any total length that fits.  Nothing is ever read
 * outside idx[0 .. nnz): each bag's lo = colptr[j]-1 and hi = colptr[j+1]-1 are clamped to
 * 0 <= lo <= hi <= nnz, and every bound that needed clamping counts one out-of-range event
 * (et_check_errors), as an index outside 1..nrows does.
 * ------------------------------------------------------------------------------- */

/* One table of a ragged lookup. */
typedef struct et_ragged_desc {
    const void* table;     /* as in et_lookup_desc */
    int64_t ld_table;
    int64_t nrows;
    int32_t dim;
    int32_t reserved;      /* 0 */
    const int64_t* idx;    /* device, the bags' indices back to back, 1-based Int64 */
    int64_t nnz;           /* entries addressable at idx (a capacity, see above) */
    const int64_t* colptr; /* device, batch + 1 entries, 1-based, non-decreasing */
    int64_t dst_row_off;   /* as in et_lookup_desc */
    int64_t cols_per_page; /* as in et_lookup_desc */
} et_ragged_desc;

/* Fused ragged lookup + concat: for every table t and bag j,
 *   dst[desc[t].dst_row_off + (0:dim_t-1), j] = table_t[:, idx_t[lo]]            (a COPY)
 *                                               + table_t[:, idx_t[lo+1]] + ...  (in order)
 * with [lo, hi) the bag's clamped range; an empty bag writes zero(T) (+0.0).  The sum starts
 * from a copy of the first row and adds the others one at a time in index order, as
 * lookup_static_inner does (src/lookup.jl:134-147), in the accumulator type of
 * et_pooled_sum (ET_FLAG_F16_FP32_ACC; BF16 in fp32 rounded once), so a bag of length L
 * equals et_pooled_sum of that bag with pool = L bit for bit, and a one-entry bag on a row
 * of -0.0 gives -0.0.  An index outside 1..nrows adds a zero row and is counted.
 * ntables <= ET_MAX_TABLES_PER_LAUNCH; a single-table ragged lookup is ntables = 1.
 * batch == 0 is a no-op.  Honours ET_FLAG_NONTEMPORAL on the stores. */
int et_ragged_maplookup_prealloc(int dtype, const et_ragged_desc* descs, int32_t ntables,
                                 int64_t batch, void* dst, int64_t ld_dst, uint32_t flags,
                                 void* stream);

/* bag[k] = 1-based bag of entry k for k in 0..nnz-1, or 0 if k lies outside
 * [colptr[0]-1, colptr[batch]-1) (the capacity tail); bounds clamped as above.  The gradient
 * column of every entry: what `map` of an Indexer built over the values (et_index_build with
 * pool = 1) is mapped through to give the reference-layout Indexer of ragged indices
 * (src/utils.jl:306-314). */
int et_ragged_bag_ids(const int64_t* colptr, int64_t batch, int64_t nnz, int64_t* bag,
                      void* stream);

/* One table of a ragged sparse-SGD update. */
typedef struct et_ragged_update_desc {
    void* table;           /* device pointer, updated in place */
    int64_t ld_table;
    int64_t nrows;
    int32_t dim;
    int32_t reserved;      /* 0 */
    const void* delta;     /* dim x batch gradient, column j at delta + j*ld_delta */
    int64_t ld_delta;
    const int64_t* idx;    /* the values of the forward lookup */
    int64_t nnz;           /* capacity of idx */
    const int64_t* colptr; /* batch + 1 entries */
    int64_t batch;
    int64_t cols_per_page; /* as in et_lookup_desc */
} et_ragged_update_desc;

/* Bytes of device workspace et_ragged_sgd needs for these descriptors (grows with the sum
 * of nnz; any alignment, as et_sgd_workspace_size). */
int et_ragged_sgd_workspace_size(const et_ragged_update_desc* descs, int32_t ntables,
                                 int64_t* bytes);

/* Sparse SGD over ragged gradients — et_sparse_sgd where entry k of a table belongs to bag
 * bag(k) (et_ragged_bag_ids) instead of bag k / pool:
 *   for every table t and every distinct column r among the entries with bag(k) != 0:
 *     acc = +0 ; for each such entry k with idx[k] == r, in INCREASING k: acc += delta_t[:, bag(k)]
 *     table_t[:, r] = the update of et_sparse_sgd (fused, ET_FLAG_SGD_UNFUSED,
 *                     ET_FLAG_SGD_F64_ALPHA)
 * — the reference's serial per-column sum (src/sparseupdate.jl:97-129) over the expanded
 * gradient, so the result equals a vector-index et_sparse_sgd of delta[:, bag(k)] bit for bit.
 * A column with no participating entry is not written; entries of the capacity tail
 * contribute nothing.  Always exact: no column is ever split (ET_FLAG_EXACT_UPDATE and
 * ET_FLAG_EXACT_IF_FAST are accepted and ignored), so a hot column is one serial chain on one
 * wave.  ET_F32 / ET_F64 / ET_F16 (both accumulation modes) / ET_BF16.
 * ET_FLAG_SGD_INDEX_ONLY, ET_FLAG_SGD_APPLY_ONLY and ET_FLAG_SGD_HOT_PASS return
 * ET_ERR_UNSUPPORTED.  Stream-ordered on the caller's stream only (no side streams, no host
 * synchronisation).  The sum of nnz must be below 2^31 - 1. */
int et_ragged_sgd(int dtype, const et_ragged_update_desc* descs, int32_t ntables, double eta,
                  uint32_t flags, void* workspace, int64_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------
 * Weighted and mean-pooled bags (EmbeddingBag's per_sample_weights and mode="mean").  The
 * reference has neither: the definitions here are the contract.
 *
 * C is the accumulator type: Float32 for ET_F32 / ET_F16 / ET_BF16 tables, Float64 for ET_F64.
 * Weights and weight gradients are ALWAYS of type C, whatever the table type.  Integer tables
 * return ET_ERR_UNSUPPORTED.  Every operation below is rounded once in C and nothing is fused
 * (the library is built with -ffp-contract=off); T(.) is one RNE rounding for 16-bit tables.
 *
 * Bags are the ragged form above: idx, colptr, the capacity nnz, the same clamping, each
 * clamped bound counted.  `weights` has the capacity of idx and entry k of idx pairs with
 * weights[k].  No kernel reads weights outside [0, nnz), or at an entry that no bag covers.
 * A fixed-pool P x B index is the ragged index with colptr = 1 + P*(0:B).
 *
 * Forward, ET_POOL_SUM, for a bag [lo, hi):
 *   an empty bag writes +0;
 *   acc = C(w_lo) * C(x_lo);  for k = lo+1 .. hi-1:  t = C(w_k) * C(x_k);  acc = acc + t
 *   out = T(acc)
 *   An index outside 1..nrows is counted and takes x = +0; it is still multiplied, so the
 *   sign of that zero follows the weight.  weights == NULL means no products: the sum starts
 *   from a COPY of the first row, and the result equals et_ragged_maplookup_prealloc (with
 *   ET_FLAG_F16_FP32_ACC for ET_F16) bit for bit.  So does the result with every weight 1.0,
 *   and a one-entry bag of weight 1.0 on a row of -0.0 gives -0.0.
 * Forward, ET_POOL_MEAN: weights must be NULL (ET_ERR_UNSUPPORTED otherwise); acc is the
 *   unweighted sum and out = T(acc / C(hi - lo)), one correctly rounded division; entries
 *   out of range count in the length; an empty bag writes +0.
 * Weight gradient: for every entry k covered by a bag j,
 *   dw[k] = sum_f C(delta[f, j]) * C(x_k[f]), formed in C; the order of the sum is the
 *   kernel's choice but the same from run to run; an index out of range gives +0; every
 *   entry of dw[0, nnz) that no bag covers is written +0 (a stream-ordered memset).  The
 *   table is read as it is when the call runs: call it before the update.
 * Weighted sparse SGD: et_ragged_sgd with a weight per entry.  For every distinct column,
 *   acc = +0; for its participating entries in increasing k:
 *   t = C(w_k) * C(delta[:, bag(k)]);  acc = acc + t;  then the update of et_sparse_sgd
 *   (fused, ET_FLAG_SGD_UNFUSED, ET_FLAG_SGD_F64_ALPHA).  Always exact, never split: one
 *   serial chain per column (a hot column costs what it costs et_ragged_sgd).  ET_F16 sums in
 *   Float32 (ET_FLAG_F16_FP32_ACC is implied and accepted).  A column with no participating
 *   entry is not written.  For ET_F32 / ET_F64 the result equals a vector-index et_sparse_sgd
 *   of the expanded gradient E[:, k] = fl_C(w_k * delta[:, bag(k)]) bit for bit.
 * Mean mode has no backward entry of its own: its pullback is the weighted update with
 * w_k = 1 / len(bag(k)).
 * ------------------------------------------------------------------------------- */
#define ET_POOL_SUM 0
#define ET_POOL_MEAN 1

/* One table of a weighted / mean lookup: et_ragged_desc with a mode and the weights. */
typedef struct et_weighted_desc {
    const void* table;     /* as in et_lookup_desc */
    int64_t ld_table;
    int64_t nrows;
    int32_t dim;
    int32_t mode;          /* ET_POOL_SUM or ET_POOL_MEAN */
    const int64_t* idx;    /* device, the bags' indices back to back, 1-based Int64 */
    int64_t nnz;           /* capacity of idx and of weights */
    const int64_t* colptr; /* device, batch + 1 entries, 1-based, non-decreasing */
    int64_t dst_row_off;   /* as in et_lookup_desc */
    int64_t cols_per_page; /* as in et_lookup_desc */
    const void* weights;   /* device, nnz entries of type C, or NULL (unweighted) */
} et_weighted_desc;

/* Fused weighted / mean lookup + concat (semantics above) into
 * dst[desc[t].dst_row_off + (0:dim_t-1), j].  Weighted, unweighted and mean tables may share
 * one call; ntables <= ET_MAX_TABLES_PER_LAUNCH; batch == 0 is a no-op.  Flags:
 * ET_FLAG_NONTEMPORAL only (any other flag: ET_ERR_UNSUPPORTED).  Every argument error (NULLs,
 * negative sizes, ld_table < dim, rows outside ld_dst, a mode that is neither, too many
 * tables; weights with ET_POOL_MEAN and integer dtypes: ET_ERR_UNSUPPORTED) is reported before
 * any device work.  Stream-ordered on the caller's stream only, allocates nothing, never
 * synchronises: capturable. */
int et_weighted_maplookup_prealloc(int dtype, const et_weighted_desc* descs, int32_t ntables,
                                   int64_t batch, void* dst, int64_t ld_dst, uint32_t flags,
                                   void* stream);

/* One table of a weighted update or weight gradient: et_ragged_update_desc, the weights and
 * the weight gradient. */
typedef struct et_weighted_update_desc {
    void* table;           /* device pointer (updated in place by et_weighted_sgd) */
    int64_t ld_table;
    int64_t nrows;
    int32_t dim;
    int32_t reserved;      /* 0 */
    const void* delta;     /* dim x batch gradient, column j at delta + j*ld_delta */
    int64_t ld_delta;
    const int64_t* idx;    /* the values of the forward lookup */
    int64_t nnz;           /* capacity of idx, weights and dweights */
    const int64_t* colptr; /* batch + 1 entries */
    int64_t batch;
    int64_t cols_per_page; /* as in et_lookup_desc */
    const void* weights;   /* type C, nnz entries: read by et_weighted_sgd only */
    void* dweights;        /* type C, nnz entries: written by et_weighted_weight_grad only */
} et_weighted_update_desc;

/* dweights[0, nnz) of every table (semantics above): reads table, delta, idx and colptr,
 * writes dweights, ignores weights.  ET_ERR_ARG before any device work: NULLs (dweights
 * included), negative sizes, a leading dimension below dim, too many tables.  Stream-ordered
 * on the caller's stream only (a memset, then the kernels), no allocation, no
 * synchronisation: capturable. */
int et_weighted_weight_grad(int dtype, const et_weighted_update_desc* descs, int32_t ntables,
                            void* stream);

/* Bytes of device workspace et_weighted_sgd needs: et_ragged_sgd_workspace_size of the same
 * sizes. */
int et_weighted_sgd_workspace_size(const et_weighted_update_desc* descs, int32_t ntables,
                                   int64_t* bytes);

/* Weighted sparse SGD (semantics above); ignores dweights.  weights == NULL of a table with
 * work is ET_ERR_ARG; ET_FLAG_SGD_INDEX_ONLY, ET_FLAG_SGD_APPLY_ONLY and ET_FLAG_SGD_HOT_PASS
 * return ET_ERR_UNSUPPORTED; ET_FLAG_EXACT_UPDATE, ET_FLAG_EXACT_IF_FAST and
 * ET_FLAG_F16_FP32_ACC are accepted and change nothing.  Stream-ordered on the caller's stream
 * only, no host synchronisation: capturable.  The sum of nnz must be below 2^31 - 1. */
int et_weighted_sgd(int dtype, const et_weighted_update_desc* descs, int32_t ntables, double eta,
                    uint32_t flags, void* workspace, int64_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------
 * Sparse AdaGrad, element-wise (Flux's ADAGrad) and row-wise, over fixed-pool and ragged
 * gradients.  The reference has no optimiser but Descent: this arithmetic is defined here,
 * and its parity with Flux is unpinned (as Float16 parity is).
 *
 * For every table t and every distinct column r with at least one participating
 * occurrence, in the accumulator type C (Float32 for F32 / F16 / BF16 tables, Float64 for
 * F64), eta_c and eps_c being eta and eps rounded to C:
 *
 *   gradient sum g.  The column's occurrence list is in occurrence order for a fixed-pool
 *   index (as et_sparse_sgd sees it) and in increasing entry k for a ragged one.  It is cut
 *   into consecutive chunks of ET_SGD_CHUNK list positions; p_c = +0, then
 *   p_c += delta[:, bag] for the chunk's occurrences in order; g = p_0 for one chunk,
 *   g = ((p_0 + p_1) + p_2) + ... in chunk order otherwise.  A column of at most ET_SGD_CHUNK
 *   occurrences is therefore the reference's serial sum (src/sparseupdate.jl:97-129); a hot
 *   column is ordered partial sums, never one serial chain.  A ragged entry with no bag (the
 *   capacity tail) adds nothing BUT KEEPS ITS LIST POSITION: the rounding of a column with
 *   more than ET_SGD_CHUNK entries depends on what sits in the tail.
 *
 *   element-wise:  s' = s + g*g ;  d = sqrt(s') + eps_c ;  w' = T(C(w) - (eta_c*g)/d)
 *   row-wise (ET_FLAG_ADAGRAD_ROWWISE): one state per column, m = (sum_f g_f^2) / dim
 *   evaluated in C (the order of that sum is the kernel's choice), s' = s + m, then d and
 *   w' as above with the scalar s'.
 *
 * Every operation is rounded once in C, nothing is contracted, sqrt and / are correctly
 * rounded, subnormals are kept; F16 / BF16 results are rounded to T once (RNE).  A column
 * with no participating occurrence is not written, and neither is its state.
 * ------------------------------------------------------------------------------- */
#define ET_FLAG_ADAGRAD_ROWWISE 512u /* et_sparse_adagrad: one accumulator per column */

/* One table of a sparse AdaGrad update: the fields of et_update_desc, the ragged form's
 * colptr / nnz, and the optimiser state. */
typedef struct et_adagrad_desc {
    void* table;           /* device pointer, updated in place */
    int64_t ld_table;
    int64_t nrows;
    int32_t dim;
    int32_t pool;          /* indices per bag of a fixed-pool index; ignored when ragged */
    const void* delta;     /* dim x batch gradient, column j at delta + j*ld_delta */
    int64_t ld_delta;
    const int64_t* idx;    /* fixed pool: the P x B indices; ragged: the values */
    int64_t ld_idx;        /* fixed pool only */
    int64_t batch;         /* bags (gradient columns) */
    int64_t cols_per_page; /* as in et_lookup_desc */
    const int64_t* colptr; /* NULL: a fixed pool.  Else batch + 1 entries, as et_ragged_desc */
    int64_t nnz;           /* ragged: capacity of idx */
    void* state;           /* device, type C, updated in place: dim x nrows with leading
                              dimension ld_state (element-wise) or nrows entries (row-wise).
                              Always ONE contiguous allocation, whatever the table's storage;
                              must not overlap the table */
    int64_t ld_state;      /* elements between the states of consecutive columns (>= dim);
                              ignored by the row-wise form */
} et_adagrad_desc;

/* Bytes of device workspace et_sparse_adagrad needs for these descriptors (grows with the
 * occurrences: pool * batch, or nnz for a ragged table; any alignment, as
 * et_sgd_workspace_size; the same for both forms and every element type). */
int et_adagrad_workspace_size(const et_adagrad_desc* descs, int32_t ntables, int64_t* bytes);

/* Sparse AdaGrad over one or many tables, fixed-pool and ragged ones in one call (semantics
 * above).  ET_F32 / ET_F64 / ET_F16 / ET_BF16 (anything else: ET_ERR_UNSUPPORTED); the table
 * and delta share the element type.  Flags: ET_FLAG_NONTEMPORAL (stores of the updated rows
 * and states) and ET_FLAG_ADAGRAD_ROWWISE; the SGD's flags (ET_FLAG_EXACT_UPDATE,
 * ET_FLAG_EXACT_IF_FAST, ET_FLAG_F16_FP32_ACC, ET_FLAG_SGD_*) return ET_ERR_UNSUPPORTED.
 * ET_ERR_ARG before any device work: a NULL state, ld_state < dim (element-wise), a state
 * that overlaps its table, negative sizes, more than ET_MAX_TABLES_PER_LAUNCH tables.
 * An index outside 1..nrows is counted (et_check_errors) and writes nothing.  Stream-ordered
 * on the caller's stream only (no side streams, no host synchronisation): capturable.
 * The occurrences of all tables together must stay below 2^31 - 1. */
int et_sparse_adagrad(int dtype, const et_adagrad_desc* descs, int32_t ntables, double eta,
                      double eps, uint32_t flags, void* workspace, int64_t ws_bytes,
                      void* stream);

/* ---------------------------------------------------------------------------------
 * Sparse AdaGrad over weighted gradients: the pullback of a weighted or mean-pooled lookup.
 * Everything of et_sparse_adagrad above holds (C, eta_c, eps_c, the element-wise and the
 * row-wise form, every operation rounded once, nothing contracted, the state layout); only
 * the gradient sum g of a table that carries weights differs.
 *
 * A weighted table is always in the ragged form: idx, colptr, the capacity nnz, the clamping
 * and counting of et_ragged_desc.  A fixed-pool (B, P) index is the ragged index with
 * colptr = 1 + P*(0:B).  `weights` has nnz entries of type C (Float32 for ET_F32 / ET_F16 /
 * ET_BF16 tables, Float64 for ET_F64) and entry k of idx pairs with weights[k].
 *
 *   gradient sum g.  The column's list is its entries in increasing k, cut into consecutive
 *   chunks of ET_SGD_CHUNK list positions.  Every chunk starts from p_c = +0; for every entry
 *   of the chunk that a bag covers, in order:  t = C(w_k) * C(delta[:, bag(k)]);
 *   p_c = p_c + t  (two roundings, never an fma).  g = p_0 for one chunk,
 *   g = ((p_0 + p_1) + p_2) + ... in chunk order otherwise: et_sparse_adagrad's rule.
 *
 * An entry that no bag covers adds nothing but keeps its list position.  Nothing is read
 * outside weights[0, nnz), and the value stored at an entry no bag covers never influences
 * any result (it need not be a valid number).  A column is participating if at least one
 * covered entry names it, WHATEVER that entry's weight: a weight of 0 still writes the column
 * and its state.  0 * Inf and 0 * NaN are NaN, as in the special-values paragraph above;
 * subnormal products are kept.
 *
 * Consequences (tests/test_gpu_weighted_adagrad.py pins them):
 *   (a) with every covered weight 1.0, table and state equal et_sparse_adagrad on the same
 *       ragged index bit for bit, element-wise and row-wise (the same g goes through the same
 *       apply step);
 *   (b) for ET_F32 / ET_F64 the result equals et_sparse_adagrad of the expanded gradient
 *       E[:, k] = fl_C(w_k * delta[:, bag(k)]) with every covered entry its own bag (entries
 *       in front of and behind the covered range stay uncovered by shifting colptr), bit for
 *       bit;
 *   (c) mean mode needs no entry of its own: its gradient carries w_k = 1 / len(bag(k)).
 * ------------------------------------------------------------------------------- */

/* One table of a weighted AdaGrad update: the fields of et_adagrad_desc, same order and
 * meaning, and the weights. */
typedef struct et_weighted_adagrad_desc {
    void* table;           /* device pointer, updated in place */
    int64_t ld_table;
    int64_t nrows;
    int32_t dim;
    int32_t pool;          /* fixed pool (weights == NULL only); ignored when ragged */
    const void* delta;     /* dim x batch gradient, column j at delta + j*ld_delta */
    int64_t ld_delta;
    const int64_t* idx;    /* fixed pool: the P x B indices; ragged: the values */
    int64_t ld_idx;        /* fixed pool only */
    int64_t batch;         /* bags (gradient columns) */
    int64_t cols_per_page; /* as in et_lookup_desc */
    const int64_t* colptr; /* NULL: a fixed pool.  Else batch + 1 entries, as et_ragged_desc */
    int64_t nnz;           /* ragged: capacity of idx and of weights */
    void* state;           /* as in et_adagrad_desc */
    int64_t ld_state;      /* as in et_adagrad_desc */
    const void* weights;   /* type C, nnz entries, or NULL */
} et_weighted_adagrad_desc;

/* Bytes of device workspace et_weighted_adagrad needs: et_adagrad_workspace_size of the same
 * sizes (the weights are read in place, no copy of them is staged). */
int et_weighted_adagrad_workspace_size(const et_weighted_adagrad_desc* descs, int32_t ntables,
                                       int64_t* bytes);

/* Sparse AdaGrad over gradients with a weight per entry (semantics above).  A table with
 * weights == NULL behaves exactly as in et_sparse_adagrad, fixed-pool or ragged; one call may
 * mix all three kinds.  weights != NULL with colptr == NULL is ET_ERR_ARG, and so are weights
 * not aligned to C.  Every other check and flag rule is et_sparse_adagrad's, reported before
 * any device work: ET_FLAG_NONTEMPORAL and ET_FLAG_ADAGRAD_ROWWISE are accepted, the SGD's
 * flags return ET_ERR_UNSUPPORTED; a NULL state, ld_state < dim (element-wise), a state that
 * overlaps its table, negative sizes and more than ET_MAX_TABLES_PER_LAUNCH tables are
 * ET_ERR_ARG.  Stream-ordered on the caller's stream only, no allocation, no host
 * synchronisation: capturable. */
int et_weighted_adagrad(int dtype, const et_weighted_adagrad_desc* descs, int32_t ntables,
                        double eta, double eps, uint32_t flags, void* workspace,
                        int64_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------
 * Split sparse SGD over ragged and weighted gradients: the opt-in counterpart of
 * et_ragged_sgd and et_weighted_sgd for skewed data.  Those two sum every column as one serial
 * chain on one wave; here a hot column is ordered partial sums of ET_SGD_CHUNK entries, as in
 * et_weighted_adagrad, followed by the update of et_sparse_sgd.  Deterministic; NOT the
 * reference's serial order for a column of more than ET_SGD_CHUNK list positions.
 *
 * Tables are et_weighted_update_desc: always the ragged form (idx, colptr, the capacity nnz,
 * the clamping and counting of et_ragged_desc).  weights == NULL is an unweighted ragged
 * gradient, otherwise `weights` has nnz entries of type C; one call may mix both kinds.
 * dweights is ignored.  C is Float32 for ET_F32 / ET_F16 / ET_BF16 tables (ET_FLAG_F16_FP32_ACC
 * is implied and accepted, as in et_weighted_sgd) and Float64 for ET_F64.
 *
 *   gradient sum g of a participating column: et_weighted_adagrad's rule, word for word.  The
 *   column's list is its entries in increasing k, cut into consecutive chunks of ET_SGD_CHUNK
 *   list positions.  Every chunk starts from p_c = +0; for every entry of the chunk that a bag
 *   covers, in order:  t = C(w_k) * C(delta[:, bag(k)]);  p_c = p_c + t  (two roundings, never
 *   an fma; a table without weights does no product at all: p_c = p_c + C(delta[:, bag(k)])).
 *   g = p_0 for one chunk, g = ((p_0 + p_1) + p_2) + ... in chunk order otherwise.
 *
 *   apply step: et_sparse_sgd's.  Fused (default): fma(-eta_c, g, w) in C, then one rounding
 *   to T;  ET_FLAG_SGD_UNFUSED: w - eta_c*g with two roundings;  ET_FLAG_SGD_UNFUSED |
 *   ET_FLAG_SGD_F64_ALPHA: evaluated in Float64 with the unconverted eta.
 *
 * An entry that no bag covers adds nothing but keeps its list position, and its weight is never
 * read.  A column participates if at least one covered entry names it, whatever that entry's
 * weight (a weight of 0 still writes the column; 0 * Inf is NaN); a column with no
 * participating entry is not written.  An index outside 1..nrows is counted (et_check_errors)
 * and writes nothing; colptr bounds are clamped and counted as in et_ragged_desc.
 *
 * Consequences (tests/test_gpu_ragged_split.py pins them):
 *   (a) a column of at most ET_SGD_CHUNK list positions gets the result of et_ragged_sgd or
 *       et_weighted_sgd bit for bit (for ET_F16: et_ragged_sgd with ET_FLAG_F16_FP32_ACC);
 *   (b) with every covered weight 1.0 the result equals weights == NULL bit for bit;
 *   (c) for ET_F32 / ET_F64 the result equals the same call on the expanded gradient
 *       E[:, k] = fl_C(w_k * delta[:, bag(k)]) with every covered entry its own bag and no
 *       weights, bit for bit;
 *   (d) mean mode needs nothing of its own: its gradient carries w_k = 1 / len(bag(k)).
 * ------------------------------------------------------------------------------- */

/* Bytes of device workspace et_ragged_sgd_split needs: et_weighted_adagrad_workspace_size of
 * the same sizes (the index workspace, a bag id per entry, the partial rows and their
 * participation flags; the weights are read in place). */
int et_ragged_sgd_split_workspace_size(const et_weighted_update_desc* descs, int32_t ntables,
                                       int64_t* bytes);

/* Split sparse SGD over ragged and weighted gradients (semantics above).  ET_F32 / ET_F64 /
 * ET_F16 / ET_BF16; anything else returns ET_ERR_UNSUPPORTED.  Flags: ET_FLAG_NONTEMPORAL (the
 * row stores), ET_FLAG_SGD_UNFUSED and ET_FLAG_SGD_F64_ALPHA select the apply step;
 * ET_FLAG_F16_FP32_ACC and ET_FLAG_EXACT_IF_FAST are accepted and change nothing;
 * ET_FLAG_EXACT_UPDATE is ET_ERR_ARG (the call is the opposite of exact);
 * ET_FLAG_SGD_INDEX_ONLY, ET_FLAG_SGD_APPLY_ONLY, ET_FLAG_SGD_HOT_PASS and
 * ET_FLAG_ADAGRAD_ROWWISE return ET_ERR_UNSUPPORTED.  ET_ERR_ARG before any device work: every
 * descriptor check of et_weighted_sgd except the NULL weights (NULL table, delta, idx or
 * colptr of a table with work, negative sizes, a leading dimension below dim, too many tables)
 * and weights not aligned to C.  Stream-ordered on the caller's stream only: no side streams,
 * no allocation, no host synchronisation, capturable.  The sum of nnz must stay below
 * 2^31 - 1. */
int et_ragged_sgd_split(int dtype, const et_weighted_update_desc* descs, int32_t ntables,
                        double eta, uint32_t flags, void* workspace, int64_t ws_bytes,
                        void* stream);

/* ---------------------------------------------------------------------------------
 * Row-wise quantised tables (inference only): INT8 or INT4 rows with a per-row Float16 scale
 * and bias, dequantised inside the pooled sum — the layout of FBGEMM's Fused8BitRowwise /
 * FusedNBitRowwise with half-precision headers.  The reference has no quantised table; the
 * definitions here are the contract.
 *
 * A quantised table is `nrows` rows; row r (1-based) starts at table + (r-1)*ld_bytes.
 *   payload  bytes [0, payload) of the row, payload = dim*bits/8.
 *            bits = 8: feature f is byte f (unsigned).
 *            bits = 4: dim is even; feature 2k is the low nibble of byte k, feature 2k+1 the
 *            high nibble.
 *   header   scale then bias, both IEEE Float16, little-endian, 4 bytes in all.
 *            fused (hdr == NULL): bytes [payload, payload+4) of the row; ld_bytes >= payload+4.
 *            split (hdr != NULL): hdr is a device array of nrows 4-byte headers;
 *            ld_bytes >= payload.
 *            In both forms ld_bytes is a multiple of 4.
 *   reads    a kernel may read any byte of [row, row + ld_bytes); it never reads outside
 *            nrows*ld_bytes of the table or nrows*4 of hdr, and no result depends on the
 *            padding bytes.
 *
 * Dequantisation, in Float32:  v_f = float(q_f)*float(scale) + float(bias).
 * q_f has at most 8 significant bits and a half has 11, so the product has at most 19 and is
 * EXACT in Float32 (24): v_f carries exactly one rounding whether the expression is evaluated
 * as a multiply and an add or as one fused multiply-add (tests/test_quant_host.py checks the
 * product against Float64 for every q and random half scales, subnormal ones included).
 *
 * Quantiser, per row; every operation is one correctly rounded Float32 operation:
 *   L = 2^bits - 1;  lo = min_f x_f;  hi = max_f x_f
 *   bias = half_rne(lo);  b = float(bias)
 *   scale = half_rne((hi - b) / L);  if float(scale) is not a finite value > 0: scale = 1.0
 *   s = float(scale);  q_f = min(max(rint((x_f - b) / s), 0), L)     (rint: ties to even)
 * A row holding a non-finite value or |x| > 65504 gets unspecified contents (never a fault);
 * so does the sign of a zero bias when the row's minimum is attained by both -0 and +0.  The
 * quantiser writes the payload and the header only, never the padding.
 *
 * Tables are contiguous only: paged quantised tables are out of scope.
 * ------------------------------------------------------------------------------- */

/* One table of a quantised lookup: fixed-pool (colptr == NULL) or ragged. */
typedef struct et_quant_desc {
    const void* table;     /* device pointer to row 1 */
    int64_t ld_bytes;      /* bytes between consecutive rows (a multiple of 4) */
    int64_t nrows;
    int32_t dim;           /* features per row */
    int32_t bits;          /* 8 or 4 */
    const void* hdr;       /* NULL: header fused in the row */
    int32_t pool;          /* fixed pool (1 = vector index); ignored when ragged */
    int32_t reserved;      /* 0 */
    const int64_t* idx;    /* fixed pool: bag j at idx + j*ld_idx; ragged: the values */
    int64_t ld_idx;        /* fixed pool only */
    const int64_t* colptr; /* NULL: a fixed pool.  Else batch + 1 entries, as et_ragged_desc */
    int64_t nnz;           /* ragged: capacity of idx */
    int64_t dst_row_off;   /* as in et_lookup_desc */
} et_quant_desc;

/* Quantise `nrows` rows of a contiguous Float32 source (row r at src + r*ld_src, ld_src >= dim)
 * into a quantised table (format and arithmetic above); hdr == NULL writes fused headers.
 * bits 8 or 4 (dim even); ld_bytes a multiple of 4 and large enough: otherwise ET_ERR_ARG. */
int et_quantize_rows(const float* src, int64_t ld_src, int64_t nrows, int32_t dim, int32_t bits,
                     void* table, int64_t ld_bytes, void* hdr, void* stream);

/* Fused pooled lookup + concat over quantised tables.  For every table t and bag j (a fixed
 * pool or a ragged bag, clamped and counted as et_ragged_desc's):
 *   acc = v(first row), a COPY; acc = acc + v(next row) one row at a time in index order, in
 *   Float32; an empty bag or pool == 0 writes +0; an index outside 1..nrows adds a zero row
 *   and is counted (et_check_errors);
 *   dst[desc[t].dst_row_off + (0:dim_t-1), j] = acc converted once (RNE) to dst_dtype
 * (ET_F32, ET_F16 or ET_BF16; anything else: ET_ERR_UNSUPPORTED).  The ET_F32 result equals
 * et_maplookup_prealloc / et_ragged_maplookup_prealloc on the dequantised Float32 table bit
 * for bit, and the 16-bit results equal et_maplookup_prealloc_to on it.  Fixed-pool and ragged
 * tables, INT8 and INT4, fused and split headers may share one call.  Rows that are whole
 * 16-byte vectors (table 16-byte aligned, ld_bytes % 16 == 0, dim*bits/8 % 16 == 0, at most
 * 1024 payload bytes) take the vector kernel, every other shape a generic one with the same
 * results.  Flags: ET_FLAG_NONTEMPORAL (the stores); any other flag: ET_ERR_UNSUPPORTED.
 * ET_ERR_ARG before any device work: bits not 8 or 4, an odd dim with 4 bits, ld_bytes too
 * small or not a multiple of 4, negative sizes, ntables > ET_MAX_TABLES_PER_LAUNCH.
 * Stream-ordered on the caller's stream only, allocates nothing, never synchronises:
 * capturable.  batch == 0 is a no-op. */
int et_quant_maplookup_prealloc(int dst_dtype, const et_quant_desc* descs, int32_t ntables,
                                int64_t batch, void* dst, int64_t ld_dst, uint32_t flags,
                                void* stream);

/* Assemble the Preallocation concat from per-rank slabs after an all-gather
 * (table-wise sharding across GPUs, no counterpart in the single-process
 * reference): slab r is a (slab_ld x batch) column-major block at
 * slabs + r*slab_ld*batch whose first rows[r] rows are copied to
 * dst[dst_row_off[r] + (0:rows[r]-1), :].  `rows`, `dst_row_off` are HOST arrays
 * of nranks entries; the rank whose slab already sits in dst can be skipped by
 * giving it rows[r] = 0. */
int et_concat_slabs(int dtype, const void* slabs, int32_t nranks, int64_t slab_ld,
                    int64_t batch, const int32_t* rows, const int64_t* dst_row_off, void* dst,
                    int64_t ld_dst, void* stream);

/* The reverse of et_concat_slabs, for the backward exchange of a sharded step:
 * slab_r[:, f] (row f < rows[r] of rank r's (slab_ld x batch) slab, slabs laid out
 * rank after rank) = src[src_row_off[r] + f, :].  Used to cut a batch-sliced gradient
 * into per-rank slabs before an all-to-all. */
int et_split_slabs(int dtype, const void* src, int64_t ld_src, int64_t batch, int32_t nranks,
                   const int32_t* rows, const int64_t* src_row_off, void* slabs,
                   int64_t slab_ld, void* stream);

/* One-sided exchange for a sharded maplookup (the "fused P2P xGMI writes" item of
 * SURVEY.md §8f rank 3; replaces the all-gather + et_concat_slabs of the concat in
 * src/lookup.jl:316-371 when every rank holds the whole destination): rows
 * col..col+ncols-1 of every bag of src ((ld x batch), this rank's finished
 * columns) are stored into the same rows of each peer destination (same ld;
 * `peers` is a HOST array of npeers device pointers from et_ipc_open).  Publish
 * with a stream-ordered barrier after the launch. */
#define ET_MAX_PEERS 16
int et_push_cols(int dtype, const void* src, int64_t ld, int64_t batch, int64_t col,
                 int64_t ncols, void* const* peers, int32_t npeers, void* stream);

/* IPC mapping of a device buffer for et_push_cols: et_ipc_handle fills `handle`
 * (64 bytes) for the allocation holding `ptr` and the byte offset of ptr in it;
 * another process maps it with et_ipc_open (peer access enabled lazily) and
 * unmaps it with et_ipc_close(ptr, offset). */
int et_ipc_handle(const void* ptr, void* handle, int64_t* offset);
int et_ipc_open(const void* handle, int64_t offset, void** ptr);
int et_ipc_close(void* ptr, int64_t offset);

/* ---------------------------------------------------------------------------------
 * Sharded PreallocationStrategy maplookup over the GPUs of a node (BASELINE config 5;
 * SURVEY.md §8e).  No counterpart exists in the single-process reference: these replace
 * the in-place concat of maplookup!(::PreallocationStrategy, dst, tables, I)
 * (src/lookup.jl:316-371, the row-block views at :334-340) when the tables are spread
 * over ranks — one process per GPU, RCCL over xGMI for the one exchange step.
 * ------------------------------------------------------------------------------- */

/* One piece of a shard plan: features [f0, f0+dim) of table `table` (0-based), owned by
 * `rank`; its rows of the destination start at `col` (prependrows included). */
typedef struct et_shard_piece {
    int32_t rank;
    int32_t table;
    int32_t f0;
    int32_t dim;
    int64_t col;
} et_shard_piece;

#define ET_PLAN_TABLEWISE 0   /* whole tables, contiguous groups balanced by count (26 tables
                                 on 8 GPUs: 4,4,3,3,3,3,3,3); with `sizes`, dealt in
                                 descending size round-robin so the largest land on
                                 distinct ranks */
#define ET_PLAN_FEATUREWISE 1 /* the concatenated feature axis cut into equal contiguous
                                 ranges at `granule`-feature boundaries inside tables, each
                                 range cut into vector-kernel widths (96 -> 64 + 32) */

/* The shard plan: every rank's pieces, rank by rank, each rank's in slab order.  With
 * out == NULL only *npieces is set (the count to allocate).  Host-only; no device. */
int et_shard_plan(int32_t mode, int32_t ntables, const int32_t* dims, const int64_t* sizes,
                  int32_t world, int64_t prependrows, int32_t granule, int32_t elsize,
                  et_shard_piece* out, int32_t cap, int32_t* npieces);

/* RCCL communicator of the ranks (one process per GPU, the current HIP device):
 * rank 0 creates a 128-byte id, the host broadcasts it by any means (MPI, a TCP store,
 * torch.distributed), every rank calls et_comm_init with it.  The comm is a
 * ncclComm_t; any ncclComm_t the host already owns may be passed instead. */
#define ET_COMM_ID_BYTES 128
int et_comm_unique_id(void* id);
int et_comm_init(void** comm, int32_t nranks, const void* id, int32_t rank);
int et_comm_destroy(void* comm);

/* A LOOPBACK communicator: nranks simulated ranks of this one process (comms[r] is rank r),
 * all on the current device, for exercising the world > 1 sharded step without nranks
 * GPUs.  Each rank must be driven by its own host thread with its own stream; every
 * collective of the sharded step (et_sharded_maplookup, et_sharded_piece_grads,
 * et_allgather_concat) is then a host rendezvous of the nranks callers followed by device
 * copies between their buffers, stream-ordered with events as RCCL orders its collectives.
 * Accepted wherever an RCCL comm is (world must equal nranks); a caller that does not
 * arrive within 120 s fails the collective.  Free each handle with et_comm_destroy. */
int et_comm_loopback(void** comms, int32_t nranks);

/* The exchange step on its own: ncclAllGather of every rank's (slab_ld x batch) slab into
 * `gathered` (nranks slabs, rank after rank), then et_concat_slabs(gathered, rows,
 * dst_row_off) into dst.  One contiguous run of destination rows per rank.  comm == NULL
 * (allowed for nranks == 1 only) copies the slab instead of calling RCCL. */
int et_allgather_concat(void* comm, int dtype, const void* slab, int64_t slab_ld, int64_t batch,
                        void* gathered, int32_t nranks, const int32_t* rows,
                        const int64_t* dst_row_off, void* dst, int64_t ld_dst, void* stream);

#define ET_EXCHANGE_ALLGATHER 0 /* every rank ends with the whole (ld_dst x batch) dst */
#define ET_EXCHANGE_ALLTOALL 1  /* DLRM layout: rank r ends with bags [r*B/N, (r+1)*B/N) of
                                   every feature (N times less on the links) */

/* A sharded step: the plan (all ranks' pieces, as from et_shard_plan), this rank, the
 * destination geometry, `chunks` batch chunks pipelined through lookup / exchange /
 * assembly (all-gather only).  comm may be NULL only for world == 1 (the exchange is then
 * a device copy).  Creates one side stream and a few events on the current device;
 * everything else is caller-owned. */
int et_sharded_create(void** handle, void* comm, int32_t world, int32_t rank, int dtype,
                      const et_shard_piece* pieces, int32_t npieces, int64_t prependrows,
                      int64_t ld_dst, int64_t batch, int32_t chunks, int32_t exchange);
/* Slab leading dimension, workspace bytes, and the bags [lo, hi) of dst this rank ends
 * with (0..batch for the all-gather). */
int et_sharded_info(void* handle, int64_t* slab_ld, int64_t* ws_bytes, int64_t* batch_lo,
                    int64_t* batch_hi);
/* One step: `local` holds this rank's pieces in plan order (table = the piece's columns,
 * e.g. a column-slice pointer with the parent's ld_table; dim = the piece's dim; idx for
 * the whole batch; dst_row_off ignored).  Stream-ordered on `stream`; dst is
 * (ld_dst x batch), or (ld_dst x (hi - lo)) for the all-to-all. */
int et_sharded_maplookup(void* handle, const et_lookup_desc* local, int32_t nlocal, void* dst,
                         int64_t ld_dst, void* workspace, int64_t ws_bytes, uint32_t flags,
                         void* stream);
/* Backward of the all-to-all layout (rrule of the sharded maplookup, src/lookup.jl:374-389):
 * from this rank's (ld_delta x (hi - lo)) gradient slice, every rank's feature rows are cut
 * out (et_split_slabs) and exchanged, giving `recv` = (slab_ld x batch): this rank's
 * pieces' gradient rows for every bag, pieces in plan order.  (Under the all-gather layout
 * the gradient is replicated and a piece's gradient is a row block of it.) */
int et_sharded_piece_grads(void* handle, const void* delta, int64_t ld_delta, void* recv,
                           void* workspace, int64_t ws_bytes, void* stream);
int et_sharded_destroy(void* handle);

/* Deterministic synthetic data (the same counter-based hash as oracle/):
 * element i of dst = lo + (hi-lo) * u(seed, offset + i), u in [0,1) with 24 bits. */
int et_fill_uniform(int dtype, void* dst, int64_t n, uint64_t seed, uint64_t offset,
                    double lo, double hi, void* stream);

/* Uniform 1-based indices in 1..nrows (hash of seed, offset + i). */
int et_fill_index_uniform(int64_t* idx, int64_t n, int64_t nrows, uint64_t seed,
                          uint64_t offset, void* stream);

/* Synchronise the device, return (and clear) the number of out-of-range indices
 * seen by any kernel since the last call. */
int et_check_errors(uint64_t* oob_count);

#ifdef __cplusplus
}
#endif

#endif /* EMBTAB_H */
