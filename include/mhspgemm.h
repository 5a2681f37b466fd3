/*
 * mhspgemm.h -- C-ABI of the MI355X-native hash-accumulator SpGEMM.
 *
 * Drop-in boundary for the reference's call path (yyssys/MH-SpGEMM):
 *   void MH_spgemm(const CSR &A, CSR &B, CSR &C, Timing &Timing, Tool &tools)
 *     (/root/reference/src/main.cu:12-72)
 * which the reference's main() calls on device-resident A and B
 * (src/main.cu:110-124) and which leaves C (C.d_ptr/d_col/d_val, C.nnz)
 * on the device.  Every entry point below is extern "C", takes plain
 * pointers and sizes, and never throws; failures return an mhs_status and
 * leave a message in mhs_last_error().
 *
 * Data contract (same as the reference):
 *   - CSR, zero-based, int32 row_ptr[M+1] / col_idx[nnz], double val[nnz].
 *   - A is M x K, B is K x N (the reference computes A*A: B = A, main.cu:101).
 *   - B's column indices are sorted ascending within each row (the reference
 *     relies on it in Form_mask_matrix_B.cuh:442-447 and guarantees it in
 *     mmio_read.h:150).  Violations are detected and reported as
 *     MHS_ERR_INVALID rather than producing a wrong C.
 *   - C's pattern is structural (cancellation zeros are kept), columns are
 *     sorted ascending per row, duplicates in A or B are summed.
 *   - Values are FP64; summation order on the GPU is not fixed, so values
 *     match a sequential reference to rounding (the north-star bound is
 *     1e-6 relative), row_ptr and col_idx match bit-exactly.  Sums are double
 *     on every FP64 path (the full call, the values plans and their backward):
 *     an entry of m kept products is within m * 2^-53 * (the sum of the
 *     products' absolute values) of the exact sum, in any order.
 *   - Inf, NaN and stored zeros propagate as IEEE arithmetic on the products does, whatever the order: every kept
 *     product is formed and nothing else is.  With each product classified in double (FP32 plans: in float; 0 * Inf
 *     and anything times NaN are NaN), an entry of C is NaN if one of its products is NaN or products of both
 *     infinities occur, +Inf or -Inf if only that infinity occurs, and otherwise finite within the bound above.  A
 *     stored zero in A or B is an ordinary entry: 0 * Inf is a NaN here as in the reference.  (Near row groups add
 *     explicit 0 * b products, so a call whose B holds a non-finite value runs without them.)  The one exemption is
 *     stated at mhs_spgemm_values_grad: a zero cotangent times a non-finite value.
 */
#ifndef MHSPGEMM_H
#define MHSPGEMM_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MHS_ABI_VERSION 10

typedef enum mhs_status {
    MHS_OK = 0,
    MHS_ERR_HIP = 1,      /* a HIP runtime call failed (reference: CHECK_ERROR throw, common.h:85-95) */
    MHS_ERR_OOM = 2,      /* device allocation failed */
    MHS_ERR_INVALID = 3,  /* bad argument, dimension mismatch, unsorted or out-of-range columns */
    MHS_ERR_OVERFLOW = 4, /* nnz(C) does not fit int32 row_ptr */
    MHS_ERR_IO = 5        /* Matrix Market read failure */
} mhs_status;

/* A CSR matrix.  For mhs_spgemm the arrays are DEVICE pointers
 * (the reference's CSR::d_ptr/d_col/d_val, inc/CSR.h:15-17). */
typedef struct mhs_csr {
    int32_t M, N, nnz;
    int32_t *ptr; /* M+1 */
    int32_t *col; /* nnz */
    double *val;  /* nnz */
} mhs_csr;

/* Per-phase times in ms, the reference's Timing fields (inc/Timing.h:3-20),
 * measured with hipEvents on the context stream, plus the two totals and
 * run statistics. */
typedef struct mhs_timing {
    double mem_alloc;          /* workspace + C.ptr allocation            */
    double Form_mask_matrix_B; /* B -> (tile col, 64-bit mask) rows       */
    double symbolic_binning;   /* row analysis + symbolic bins            */
    double Calculate_C_nnz;    /* symbolic: nnz of every C row            */
    double numeric_binning;    /* row_ptr scan + numeric bins + readback  */
    double Malloc_C_col_val;   /* C.col / C.val allocation                */
    double Numeric;            /* numeric: values + sorted columns        */
    double total_ref;          /* = getTotal(): all but Form_mask_matrix_B (src/Timing.cpp:39-41) */
    double total_e2e;          /* everything, device-resident A,B -> device-resident C */
    uint64_t flop;             /* sum over A's nonzeros of nnz(B row)   (src/main.cu:102-107) */
    int64_t nnzC;
    int32_t sym_bins[16];      /* rows per symbolic bin (0: rows not processed: empty, or in a row group) */
    int32_t num_bins[16];      /* rows per numeric bin  (0: likewise)                                  */
} mhs_timing;

typedef struct mhs_ctx mhs_ctx;

/* Context = the reference's Tool (inc/Tool.h, src/Tool.cu:4-45): stream,
 * workspace (kept across calls, grown on demand), pinned readback area.
 * One context per device; a context is not thread-safe, distinct contexts
 * may be used from distinct threads. */
int mhs_ctx_create(mhs_ctx **ctx, int device);
void mhs_ctx_destroy(mhs_ctx *ctx);
const char *mhs_last_error(const mhs_ctx *ctx);
/* Run on a caller-owned hipStream_t (e.g. PyTorch's current stream); NULL
 * restores the context's own stream. */
int mhs_ctx_set_stream(mhs_ctx *ctx, void *hip_stream);
/* The device's default (null) stream has the handle NULL and so cannot be given to mhs_ctx_set_stream:
 * NULL selects the context's own stream, which is non-blocking -- it has no order against the null
 * stream.  A caller whose data is produced or consumed on the null stream (PyTorch's default stream)
 * and who runs unsynchronised calls (MHS_OPT_SYNC 0) fences them with this: after == 0, before the
 * call: the context stream waits for everything queued on the null stream so far; after == 1, after
 * the call: the null stream waits for everything queued on the context stream so far.  Two event
 * operations, no host synchronisation.  An addition to ABI version 10: look the symbol up before use. */
int mhs_ctx_fence_default_stream(mhs_ctx *ctx, int after);
/* Release cached workspace and pooled output buffers. */
int mhs_ctx_trim(mhs_ctx *ctx);

/* Context options (mhs_ctx_set_option):
 *   MHS_OPT_SYNC (default 1): mhs_spgemm returns after C is complete.  0: it
 *     returns once the numeric phase is queued on the context stream (C's
 *     nnz and arrays are valid; their contents are stream-ordered, as for any
 *     kernel output).  A call with a timing struct always synchronises.
 *   MHS_OPT_NUMERIC_EVENTS (default 0): keep hipEvent pairs around the numeric
 *     phase of the last `value` calls, read with mhs_ctx_numeric_ms.
 *   MHS_OPT_MEM_BUDGET (default 0 = none): treat a call's workspace, or workspace
 *     plus C, beyond `value` MiB as an out-of-memory condition (exercises the
 *     row-chunked fallback below without filling the device).
 *   MHS_OPT_TINY_FIRST_ROWS (default 524288; < 0: never): from this many rows of A
 *     on, rows of at most 128 products are summed during the symbolic phase into
 *     cached value slots and numeric only copies them into C (one sort instead of
 *     two; one more device-to-host hand-off per call, so big matrices only).  Below
 *     the threshold, matrices averaging fewer than 12 entries a row take the same
 *     path without the hand-off, with slots sized by the per-row bound (M * 128 *
 *     12 bytes, cached in the context; skipped when they do not fit the device or
 *     MHS_OPT_MEM_BUDGET).  A negative value turns both off.
 *   MHS_OPT_SPECULATE (default 1; env MHS_NO_SPEC=1 sets 0): a call on the same
 *     operands as the context's previous call (the same device arrays and sizes)
 *     queues the previous call's numeric launches behind the row_ptr scan instead of
 *     waiting for its statistics; the scan checks on the device that the call's
 *     statistics equal the plan's, the numeric kernels run only then, and a
 *     mismatch reruns the call without speculation (MHS_STAT_SPEC_MISS).  Every
 *     phase runs on every call either way.
 *   MHS_OPT_GROUP_GRID (default 0 = derived; env MHS_GROUP_GRID): block cap of the
 *     grouped numeric launch (rows of one column pattern, three FEM dofs of a node,
 *     processed together).  By default a bin of more row groups than the device's
 *     resident waves launches that resident set (compute units x 4 blocks) and its
 *     waves loop over the groups -- static rounds, the last ones drawn from row
 *     cursors -- while smaller bins launch a wave a group.  A value > 0 makes every
 *     grouped launch loop on at most `value` blocks (rounded up to a multiple of 8):
 *     for tests, so that a small matrix exercises the loop.  Results do not depend
 *     on it.  An ABI addition: MHS_ABI_VERSION stays 10.
 * Out of memory: when the workspace, C.ptr, the global-bin scratch or C beside them does
 * not fit, mhs_spgemm gives back every cached buffer and retries row-chunked: a counting
 * pass with the largest chunk workspace that fits sizes C; C is allocated before the
 * second pass's workspace (halved only while that workspace does not fit beside C).  It
 * returns MHS_ERR_OOM right after the counting pass when C itself does not fit, or when
 * a one-row workspace does not fit. */
typedef enum mhs_option { MHS_OPT_SYNC = 1, MHS_OPT_NUMERIC_EVENTS = 2, MHS_OPT_MEM_BUDGET = 3,
                           MHS_OPT_TINY_FIRST_ROWS = 4, MHS_OPT_SPECULATE = 5, MHS_OPT_GROUP_GRID = 6 } mhs_option;
int mhs_ctx_set_option(mhs_ctx *ctx, int option, int value);
/* Calls of this context that ran row-chunked (the out-of-memory fallback). */
long long mhs_ctx_chunked_calls(const mhs_ctx *ctx);
/* Path counters of this context (diagnostics, ABI v9): calls that ran
 *   MHS_STAT_CHUNKED      row-chunked (as mhs_ctx_chunked_calls),
 *   MHS_STAT_SPLIT        their numeric block bins split by LDS need (k_split_bins),
 *   MHS_STAT_SYM_FORK     the rare symbolic bins on an aux stream beside the common ones,
 *   MHS_STAT_NFT          numeric-first tiny rows (value slots filled by the symbolic pass),
 *   MHS_STAT_NEAR         near row groups verified (union rows built),
 *   MHS_STAT_MULTI_STREAM numeric launches dealt over several streams,
 *   MHS_STAT_SPEC         (ABI v10) the previous call's numeric plan launched ahead of the scan,
 *   MHS_STAT_SPEC_MISS    ... and rejected by the scan (the call reran without speculation),
 *   MHS_STAT_SPEC_SKIPPED symbolic launches left out by speculated calls (the plan's empty bins),
 *   MHS_STAT_WIDE_OFFSETS (an addition to ABI v10) their numeric kernels with 64-bit byte offsets into
 *                         B's arrays: nnz(B) + 3 nnz(A) >= 2^29, or every call of a context created
 *                         with the environment variable MHS_NO_O32=1 (a test switch: small operands
 *                         run the kernels of huge ones).  Once per call, also after a speculation miss.
 *   MHS_STAT_POISON_FILLS (an addition to ABI v10) not calls but fills: the buffers a context created with
 *                         the environment variable MHS_POISON=<byte, 0..255> has filled with that byte
 *                         (a test switch: every device buffer the library allocates for its own work, every
 *                         buffer its output pool hands out, and the cached workspace at the start of every
 *                         attempt of mhs_spgemm, so that nothing a call reads without writing it first holds
 *                         what an earlier call left).  0 without the variable.
 * Returns -1 for a null context or an unknown counter. */
typedef enum mhs_stat { MHS_STAT_CHUNKED = 0, MHS_STAT_SPLIT = 1, MHS_STAT_SYM_FORK = 2, MHS_STAT_NFT = 3,
                        MHS_STAT_NEAR = 4, MHS_STAT_MULTI_STREAM = 5, MHS_STAT_SPEC = 6, MHS_STAT_SPEC_MISS = 7,
                        MHS_STAT_SPEC_SKIPPED = 8, MHS_STAT_WIDE_OFFSETS = 9, MHS_STAT_POISON_FILLS = 10 } mhs_stat;
long long mhs_ctx_stat(const mhs_ctx *ctx, int which);
/* Numeric-phase durations (ms) of the last min(n, recorded) calls, oldest
 * first; waits for them.  Returns the count written, or -status on error. */
int mhs_ctx_numeric_ms(mhs_ctx *ctx, float *out, int n);

/* Hash probe conflicts (the reference's HASH_CONFLICT switch, inc/common.h:18, printed
 * at src/main.cu:68-71): probe steps that met another key in the symbolic and numeric
 * tile hash tables (inserts and lookups) since the previous call of this function, which
 * resets the count.  Only the diagnostic library libmhspgemm_probe.so (built with
 * MHS_PROBE_STATS=1) counts; the product library returns MHS_ERR_INVALID.  Synchronises
 * the context stream.  The counter is per process (shared by all contexts). */
int mhs_probe_conflicts(mhs_ctx *ctx, uint64_t *count);

/* C = A * B on the device.  A, B: device CSR.  On MHS_OK, C->M = A->M,
 * C->N = B->N, C->nnz is set and C->ptr/col/val are fresh device
 * allocations owned by the caller (free with mhs_csr_free, or hand back to
 * the context's pool with mhs_ctx_recycle).  A and B may alias.  B is not
 * modified (unlike the reference, which allocates B.d_tile* in place).
 * Returns after C is complete (the context stream is synchronised), unless
 * MHS_OPT_SYNC is 0.  t may be NULL. */
int mhs_spgemm(mhs_ctx *ctx, const mhs_csr *A, const mhs_csr *B, mhs_csr *C, mhs_timing *t);

/* ---- values-only SpGEMM: recompute C's values on a kept pattern -----------
 * (the "reuse" / compute stage of the vendor libraries' SpGEMM).  For callers that repeat one
 * product on fixed patterns with new values (time steppers, Newton loops, AMG set-up): the
 * pattern phases of mhs_spgemm, the allocation of C and the host hand-off are paid once, at
 * plan creation.  These entry points are additions to ABI version 10: nothing declared above
 * changes, so MHS_ABI_VERSION stays 10 and binaries built against the earlier header keep
 * working; callers that may meet an older library look the symbols up before use. */
typedef struct mhs_values_plan mhs_values_plan;

/* Build once per pattern.  A, B, C: device CSR; C->ptr / C->col hold a pattern that
 * contains the pattern of A*B (normally C from mhs_spgemm on operands of this pattern).
 * The plan borrows the six pattern arrays (A/B/C ptr and col): the caller keeps them alive
 * and unchanged until the plan is destroyed.  No val array is read.  Synchronous.
 * Validated here, on the device, once: A.N == B.M, C.M == A.M, C.N == B.N; the three row_ptr
 * arrays monotone from 0 to nnz; A's columns < B.M; C's columns strictly ascending and in
 * range within each row; every product's column present in its C row.  A violation returns
 * MHS_ERR_INVALID with a message naming the first bad row, and no plan.
 * The plan owns its device memory (row lists of about M ints, counters, a status word), not
 * the context workspace: mhs_spgemm calls and mhs_ctx_trim on the same context leave it alone. */
int mhs_values_plan_create(mhs_ctx *ctx, const mhs_csr *A, const mhs_csr *B, const mhs_csr *C,
                           mhs_values_plan **plan);
/* Cval[Cptr[i]..Cptr[i+1]) = values of row i of A*B at C's columns; entries of C's pattern
 * that no product reaches get 0.0.  Aval/Bval/Cval: device arrays of nnz(A)/nnz(B)/nnz(C)
 * doubles, any buffers (Cval may be C->val or another array).  ms == NULL: follows
 * MHS_OPT_SYNC like mhs_spgemm (0: returns once queued on the context stream).  ms != NULL:
 * synchronises and writes the hipEvent time of the call.
 * Hot calls do not re-validate: the pattern arrays must not have changed since plan creation.
 * A call with ms == NULL and MHS_OPT_SYNC 0 allocates nothing, reads nothing back and does not
 * synchronise; it only launches on the context stream (mhs_ctx_set_stream's, when set).
 * Non-finite values and stored zeros follow the data contract at the top of this header -- on every plan: plain or
 * masked in any form (a product outside the mask reaches no entry, finite or not), either value type, any width
 * and every set of a batched call (a set's Inf or NaN stays in that set), forward and backward. */
int mhs_spgemm_values(mhs_ctx *ctx, mhs_values_plan *plan, const double *Aval, const double *Bval,
                      double *Cval, double *ms);
typedef struct mhs_values_info {
    int32_t rows[8];              /* rows per class, index = class id (0: nothing to compute; 1 team, 2 wave-direct,
                                   * 3 wave-search, 4 block-direct, 5 block-search, 6 global; 7 dot: masked plans) */
    int64_t products, nnzC, plan_bytes;
} mhs_values_info;
int mhs_values_plan_info(const mhs_values_plan *plan, mhs_values_info *info);
/* Frees the plan's device memory (waits for the context stream first).  NULL plan: no-op. */
void mhs_values_plan_destroy(mhs_ctx *ctx, mhs_values_plan *plan);

/* ---- masked product: C<M> = A*B on a given pattern --------------------------
 * For callers whose pattern is smaller than the product's (triangle counting L*L on L, ILU(0)- and
 * SPAI-style updates on A's pattern, sparsified AMG coarse operators).  C->ptr / C->col are the mask:
 * for every mask entry (i, j), Cval = sum_k A_ik * B_kj; duplicates in A and in B are summed, a mask
 * entry no product reaches gets exactly 0.0, products whose column is not in the mask row are dropped.
 * Complemented and value-dependent masks are not supported.  The result is an ordinary
 * mhs_values_plan: mhs_spgemm_values, mhs_values_plan_info and mhs_values_plan_destroy run it as they
 * run any other.  Validation is mhs_values_plan_create's (dimensions, the three row_ptr arrays, A's
 * columns < B.M, C's columns strictly ascending in range) without the containment check; B's columns
 * are checked to lie in [0, B.N) when B^T is built.  A's rows need not be sorted; B's are ascending.
 * form says how rows are computed:
 *   MHS_MASK_PRODUCT  every row walks its products and drops the misses (the classes 1..6 above)
 *   MHS_MASK_DOT      every row with mask and A entries takes the inner-product form (class 7): per
 *                     mask entry (i, j), A's row i is intersected with B's column j.  Its sum order
 *                     is fixed -- A's entry order, then B's duplicate order -- so two calls give the
 *                     same bits on these rows.
 *   MHS_MASK_AUTO     per row, the dot form where its search steps, weighted, are fewer than the
 *                     row's products
 * The dot form reads B^T's pattern: built at creation for AUTO and DOT, kept (4 (B.N + 1) + 8 nnz(B)
 * bytes of the plan's own memory, part of plan_bytes) only while some row uses it.  Any other form
 * value: MHS_ERR_INVALID.  Additions to ABI version 10, like the entries above. */
typedef enum mhs_mask_form { MHS_MASK_AUTO = 0, MHS_MASK_PRODUCT = 1, MHS_MASK_DOT = 2 } mhs_mask_form;
int mhs_values_plan_create_masked(mhs_ctx *ctx, const mhs_csr *A, const mhs_csr *B, const mhs_csr *C,
                                  int form, mhs_values_plan **plan);
/* The products that land in the plan's C pattern (mhs_values_info::products counts them all).
 * A plan of mhs_values_plan_create: kept == products. */
int mhs_values_plan_kept(const mhs_values_plan *plan, int64_t *kept_products);

/* ---- the backward of a values call: gradients of Aval and Bval on a kept plan -------------
 * For callers that differentiate through the product on fixed patterns (adjoint sensitivities of a
 * Galerkin product, learned AMG or sparsifiers, a sparse-sparse product inside a PyTorch model).
 * (Aval, Bval) -> Cval is bilinear; with dCval the cotangent on the plan's C pattern (nnz(C) doubles),
 *   dAval[p] = sum over B's row k of Bval[(k,j)] * dCval[slot(i,j)]          for the A entry p = (i,k)
 *   dBval[q] = sum over the A entries (i,k) of Aval[(i,k)] * dCval[slot(i,j)] for the B entry q = (k,j)
 * Duplicates in B each contribute to dAval, duplicates in A each get their own (equal) gradient and each
 * contribute to dBval.  On a masked plan a product whose column is not in the mask row contributes to
 * neither.  dAval: nnz(A) doubles, dBval: nnz(B) doubles; either may be NULL (that side is not computed),
 * not both.  Bval is read only when dAval is given and Aval only when dBval is given; the unused one may
 * be NULL.  Outputs must not alias inputs.  Every entry of a requested output is written: an entry that
 * no kept product reaches (an empty B row, an empty C row, a B row no A column points at) gets exactly 0.0.
 * dAval is summed without atomics in a fixed order: two calls give the same bits.  dBval is summed by
 * FP64 atomics: its order is not fixed.  Inf, NaN and stored zeros in Aval, Bval and dCval propagate as the data
 * contract at the top says, with one exemption: a zero cotangent times a non-finite value may give 0 or NaN.
 * ms and MHS_OPT_SYNC as in mhs_spgemm_values: a call with ms == NULL and MHS_OPT_SYNC 0 allocates nothing,
 * reads nothing back and does not synchronise; it queues a zero fill of the outputs and the kernels on
 * the context stream.  Hot calls do not re-validate.  NULL ctx, plan or dCval, both outputs NULL, or a
 * needed input NULL: MHS_ERR_INVALID before any HIP call.  Any plan will do (mhs_values_plan_create or
 * _masked, any form).  An addition to ABI version 10, like the entries above. */
int mhs_spgemm_values_grad(mhs_ctx *ctx, mhs_values_plan *plan, const double *Aval, const double *Bval,
                           const double *dCval, double *dAval, double *dBval, double *ms);

/* ---- FP32 values plans: forward, masked and backward on float values -------------------------
 * For callers whose values are float (a sparse-sparse product inside a float32 model): no casts around the
 * call, half the value bytes, and rows in cheaper classes -- a plan's classes are LDS arithmetic on the
 * value's size (FP32: a wave holds 2048 direct columns or 1024 searched entries, a block 39,936 or 19,968).
 * A plan has one value type, fixed at creation: classes, row lists and both launch plans are computed for
 * it.  mhs_values_plan_create_typed with MHS_F64 is exactly mhs_values_plan_create (masked == 0; form is
 * then ignored) or mhs_values_plan_create_masked (masked != 0); any other dtype: MHS_ERR_INVALID.  Plan
 * creation reads no val array, so the mhs_csr arguments serve as they are, whatever their val points at.
 * mhs_spgemm_values_f32 and mhs_spgemm_values_grad_f32 are mhs_spgemm_values and mhs_spgemm_values_grad on
 * float arrays: the same null handling, ms and MHS_OPT_SYNC, no allocation and no read-back in a hot call,
 * every entry of a requested output written, entries no kept product reaches exactly 0.0f.  Sums are float:
 * an entry of m kept products is within m * 2^-24 * (the sum of the products' absolute values) of the exact
 * sum, in any order; LDS and memory atomics may flush subnormal sums to zero.  dAval keeps its fixed order
 * (two calls give the same bits), dBval is summed by FP32 atomics.
 * A call of the wrong type -- an _f32 call on an FP64 plan, a double call on an FP32 plan -- returns
 * MHS_ERR_INVALID with a message naming both types, before any HIP call; nothing is written.
 * Cost on MI355X: the backward gains from the halved value bytes; the forward does not
 * where LDS sums carry the call (many products per C entry) -- the LDS float add is far slower than the
 * double one there, and such an FP32 forward is slower than the FP64 forward of the same pattern.  The remedy is a
 * mixed plan, float values summed in double (mhs_values_plan_create_accum with MHS_ACC_F64, below; DESIGN section 19:
 * 0.22x the FP32 forward on cant-like, 1.04x the FP64 one).
 * Additions to ABI version 10, like the entries above. */
typedef enum mhs_dtype { MHS_F64 = 0, MHS_F32 = 1 } mhs_dtype;
int mhs_values_plan_create_typed(mhs_ctx *ctx, const mhs_csr *A, const mhs_csr *B, const mhs_csr *C,
                                 int masked, int form, int dtype, mhs_values_plan **plan);
/* The plan's value type (mhs_dtype). */
int mhs_values_plan_dtype(const mhs_values_plan *plan, int *dtype);
int mhs_spgemm_values_f32(mhs_ctx *ctx, mhs_values_plan *plan, const float *Aval, const float *Bval,
                          float *Cval, double *ms);
int mhs_spgemm_values_grad_f32(mhs_ctx *ctx, mhs_values_plan *plan, const float *Aval, const float *Bval,
                               const float *dCval, float *dAval, float *dBval, double *ms);

/* ---- batched values calls: several value sets in one walk of the pattern ---------------------
 * For callers with nb value sets on one pattern triple (the heads of a sparse attention layer, an ensemble
 * over one mesh, a batch of matrices from one stencil, many A's against one fixed B).  A plan has a third
 * fixed property beside its value type, its width W (1, 2 or 4): the value sets one walk of the patterns
 * sums.  The pattern work of a product -- the B column, the A entry, the slot in C's row -- is done once for
 * W sets, only the value loads and the sums W times.  A row's class is LDS arithmetic on the sum bytes
 * W * sizeof(value): at 16 B (FP64 W=2, FP32 W=4) a wave holds 512 direct columns or 408 searched entries and
 * a block 9,984 or 7,986; at 32 B (FP64 W=4) 256 / 226 and 4,992 / 4,436 (FP32 W=2 is the FP64 table).
 * Rows therefore move to costlier classes as W grows.  Cost on MI355X against nb unbatched calls (DESIGN section
 * 14, nb = 8): where loads and searches carry the call batching divides it (scircuit-like 0.64x at W = 2, 0.49x at
 * FP32 W = 4; masked triangle 0.6x, 0.33x at FP32 W = 4); where one LDS add per product and set carries it there is
 * only the walk to save (cant-like W = 2: 0.99x), and FP64 W = 4 is then 1.5x slower than the loop -- its
 * block-direct rows declare four times the LDS of the unbatched launch and run on wider kernels.  Use W <= 2 on
 * such patterns.
 * mhs_values_plan_create_batched with width 1 is exactly mhs_values_plan_create_typed; a width other than
 * 1, 2 or 4 returns MHS_ERR_INVALID before any HIP call.  Validation, borrowing and plan memory as for any plan.
 * mhs_spgemm_values_batched / _f32: set b (0 <= b < nb) reads Aval + b * strideA and Bval + b * strideB and
 * writes Cval + b * strideC.  Strides are in elements.  An input stride of 0 means one array shared by all
 * sets; otherwise it is >= that matrix's nnz.  strideC >= nnz(C) whenever nb > 1.  Outputs must not overlap
 * inputs or each other.  Every set has the contract of the unbatched call: every entry written, entries no
 * kept product reaches exactly 0, the any-order bound of the plan's type, the data contract's propagation of Inf,
 * NaN and stored zeros within the set (a set's non-finite values reach no other set).  Nothing outside the nb segments of
 * nnz(C) values is written.  On the dot rows of a masked plan a set has the bits of the unbatched call on its
 * values.  Any nb >= 1 runs on any plan: ceil(nb / W) passes of the plan's launch list, the last with the
 * remaining sets (on a width-1 plan: nb runs of the unbatched kernels).  mhs_spgemm_values / _f32 on a plan of
 * any width is the nb = 1 batched call.  ms and MHS_OPT_SYNC as in mhs_spgemm_values (a timed call brackets
 * all passes); with ms == NULL and MHS_OPT_SYNC 0 the call allocates nothing, reads nothing back and does not
 * synchronise.  Refused with MHS_ERR_INVALID and a message before any HIP call, writing nothing: nb < 1, a
 * negative stride, an input stride between 1 and nnz - 1, strideC < nnz(C) with nb > 1, a needed array NULL,
 * a call of the wrong type, a plan of another device.  mhs_spgemm_values_grad / _f32 on a plan of width > 1 is
 * refused likewise (those two entry points serve width-1 plans); the backward of a batched call on a plan of any
 * width is mhs_spgemm_values_grad_batched, below.
 * Additions to ABI version 10, like the entries above. */
#define MHS_VAL_WIDTH_MAX 4
int mhs_values_plan_create_batched(mhs_ctx *ctx, const mhs_csr *A, const mhs_csr *B, const mhs_csr *C,
                                   int masked, int form, int dtype, int width, mhs_values_plan **plan);
/* The plan's width. */
int mhs_values_plan_width(const mhs_values_plan *plan, int *width);
int mhs_spgemm_values_batched(mhs_ctx *ctx, mhs_values_plan *plan, int nb,
                              const double *Aval, int64_t strideA, const double *Bval, int64_t strideB,
                              double *Cval, int64_t strideC, double *ms);
int mhs_spgemm_values_batched_f32(mhs_ctx *ctx, mhs_values_plan *plan, int nb,
                                  const float *Aval, int64_t strideA, const float *Bval, int64_t strideB,
                                  float *Cval, int64_t strideC, double *ms);

/* ---- the backward of a batched values call: W cotangent sets in one walk of the pattern -------
 * The adjoint of mhs_spgemm_values_batched, for the same callers when they train or compute sensitivities.  It
 * runs on a plan of any width W: the pattern work of a product -- the B column, the slot in C's row, the staged
 * B-row bounds -- is done once for W sets, the value loads, the register sums of dAval and the atomics of dBval W
 * times.  The LDS a class holds W sums per C entry in holds W cotangents per C entry here, so the classes are the
 * forward's.
 * Set b (0 <= b < nb) reads Aval + b * strideA, Bval + b * strideB and dCval + b * strideG and writes
 * dAval + b * strideDA and dBval + b * strideDB.  Strides are in elements.  strideA and strideB follow the
 * forward's rule (0: one array shared by all sets, otherwise >= that matrix's nnz).  strideG >= nnz(C),
 * strideDA >= nnz(A) and strideDB >= nnz(B) whenever nb > 1; 0 is not taken for them: gradients always come back
 * per set, and the gradient of a shared operand is the caller's sum of them.  Per set everything is
 * mhs_spgemm_values_grad's contract: either output may be NULL, not both; Bval is read only for dAval and Aval
 * only for dBval, and the unused one may be NULL; every entry of a requested output segment is written, entries
 * no kept product reaches exactly 0; masked plans of all three forms are served; dBval is summed by atomics in
 * any order; dAval has no atomics and a fixed order -- two calls give the same bits, a set gives the same bits
 * inside any batch and alone, and on finite values without underflow they are the bits of mhs_spgemm_values_grad
 * on a width-1 plan of the same type with that set's values.  Nothing outside the nb segments is written: padding
 * between strided sets keeps its bytes.  Outputs must not overlap inputs or each other.
 * Any nb >= 1 runs on any plan: ceil(nb / W) passes of the backward's launch list, the last with the remaining
 * sets (on a width-1 plan: nb runs of the unbatched kernels).  ms and MHS_OPT_SYNC as in mhs_spgemm_values (a
 * timed call brackets all passes); with ms == NULL and MHS_OPT_SYNC 0 the call allocates nothing, reads nothing
 * back and does not synchronise: it queues one zero fill per requested side, over the nb segments only, and the
 * kernels.  Cost on MI355X against nb unbatched backward calls on a width-1 plan (nb = 8): where
 * loads and searches carry the call batching divides it (scircuit-like 0.60-0.80x at W = 2, 0.40-0.59x at FP32 W = 4;
 * masked triangle 0.58-0.61x at W = 2, 0.33-0.35x at FP32 W = 4, on either side and on both).  dBval on cant-like is
 * its atomics at every width (0.95-1.00x).  Slower than the loop there: dAval alone at FP64 W = 4 (1.59x; W = 2
 * 1.02x, FP32 W = 2 1.09x) and the two-sided FP64 W = 4 call (1.01x); and on scircuit-like FP64 W = 4 dBval and the
 * two-sided call (1.08x).  Use W <= 2 for FP64 on such patterns.
 * Refused with MHS_ERR_INVALID and a message before any HIP call, writing nothing: nb < 1, a negative stride, an
 * input stride between 1 and nnz - 1, strideG / strideDA / strideDB below its nnz with nb > 1, NULL dCval, both
 * outputs NULL, a needed input NULL, a call of the wrong type, a plan of another device.
 * Additions to ABI version 10, like the entries above. */
int mhs_spgemm_values_grad_batched(mhs_ctx *ctx, mhs_values_plan *plan, int nb,
                                   const double *Aval, int64_t strideA, const double *Bval, int64_t strideB,
                                   const double *dCval, int64_t strideG,
                                   double *dAval, int64_t strideDA, double *dBval, int64_t strideDB, double *ms);
int mhs_spgemm_values_grad_batched_f32(mhs_ctx *ctx, mhs_values_plan *plan, int nb,
                                       const float *Aval, int64_t strideA, const float *Bval, int64_t strideB,
                                       const float *dCval, int64_t strideG,
                                       float *dAval, int64_t strideDA, float *dBval, int64_t strideDB, double *ms);

/* ---- semiring values plans: min-plus, max-plus and max-min on a kept pattern ------------------
 * For graph callers: one relaxation step of shortest paths (min-plus: A (x) A on a kept pattern, or masked on A's
 * own pattern to tighten existing edges only), longest or critical paths and Viterbi-style scoring (max-plus),
 * widest (bottleneck) paths (max-min; on {0, 1} values the boolean or-and product, i.e. reachability).  A plan has a
 * fourth fixed property beside its value type, its width and its mask form: its semiring (add, mul, the identity
 * of add):
 *   MHS_SR_PLUS_TIMES   +    x    0       every plan of the creation calls above
 *   MHS_SR_MIN_PLUS     min  +    +Inf
 *   MHS_SR_MAX_PLUS     max  +    -Inf
 *   MHS_SR_MAX_MIN      max  min  -Inf
 * mhs_values_plan_create_semiring with MHS_SR_PLUS_TIMES is exactly mhs_values_plan_create_typed; any other semiring
 * value returns MHS_ERR_INVALID before any HIP call.  Semiring plans have width 1.  Validation, borrowing, plan
 * memory, mhs_values_plan_info and mhs_values_plan_kept are those of any plan; a row's class is LDS arithmetic on
 * the value's size and does not depend on the semiring, nor do the masked forms and AUTO's rule.
 * Hot calls are the entry points above -- mhs_spgemm_values, _f32, mhs_spgemm_values_batched, _batched_f32 (nb runs
 * of the kernels, as on any width-1 plan) -- with their stream, ms, MHS_OPT_SYNC and no-allocation contract; the plan
 * knows its semiring.  On a plan of one of the three new semirings:
 *   Cval(i,j) = add over the kept products of mul(A(i,k), B(k,j)).
 *   Every duplicate entry of A or B is a product of its own: duplicates are reduced by add, not summed.
 *   On a masked plan a product outside the mask reaches nothing.
 *   Every entry of the C segment is written; an entry that no kept product reaches gets the identity of add:
 *   +Inf, -Inf or -Inf.
 *   Results are bit-identical to any sequential evaluation in the plan's value type, in any order, on every class
 *   (min and max are exact and the one rounding of a + b does not depend on order), and so from call to call; the one
 *   exemption is that the sign of a zero result is unspecified.
 *   +-Inf values are ordinary: +Inf is "no edge" under min-plus.
 *   A product that is NaN leaves that entry unspecified: either NaN or the add of its other products (the hardware
 *   min and max are minNum and maxNum).  A NaN product comes from a NaN operand, or from +Inf + -Inf under the two
 *   _PLUS semirings.  No other entry is affected.
 *   FP32: a subnormal product or result may be flushed to zero, as on FP32 plus-times plans.
 * The four backward entry points (mhs_spgemm_values_grad, _f32, _grad_batched, _grad_batched_f32) on a plan whose
 * semiring is not MHS_SR_PLUS_TIMES return MHS_ERR_INVALID before any HIP call, with a message naming the semiring,
 * and write nothing: min and max have subgradients only, which mhs_spgemm_values_subgrad computes (next section).
 * Cost on MI355X: DESIGN section 16.  Additions to ABI version 10, like the entries above. */
typedef enum mhs_semiring { MHS_SR_PLUS_TIMES = 0, MHS_SR_MIN_PLUS = 1, MHS_SR_MAX_PLUS = 2, MHS_SR_MAX_MIN = 3 } mhs_semiring;
int mhs_values_plan_create_semiring(mhs_ctx *ctx, const mhs_csr *A, const mhs_csr *B, const mhs_csr *C,
                                    int masked, int form, int dtype, int semiring, mhs_values_plan **plan);
/* The plan's semiring (mhs_semiring). */
int mhs_values_plan_semiring(const mhs_values_plan *plan, int *semiring);

/* ---- semiring subgradients: the backward of min-plus, max-plus and max-min plans -------------
 * For the same callers when the tropical product sits inside a differentiable program: differentiable dynamic
 * programming, learned edge weights under a shortest-path loss, structured prediction with a hard max.  min and max
 * have subgradients only; this is the one the library computes.  On a plan of semiring MHS_SR_MIN_PLUS, _MAX_PLUS or
 * _MAX_MIN, Cval is the forward result for (Aval, Bval) and G = dCval.  A kept product (p, q, s) has A entry p, B
 * entry q and C slot s.
 *   Winner.  A product is a winner of s when mul(Aval[p], Bval[q]) == Cval[s], compared as values in the plan's
 *   type, and Cval[s] is not the identity of add.  So an entry that equals the identity has no winners and passes
 *   nothing: an entry no product reaches, and also "no path" (every product +Inf under min-plus).  A NaN never
 *   compares equal: a NaN product is never a winner and a NaN Cval[s] has no winners.  The forward is bit-identical
 *   to a sequential evaluation and the backward forms mul with the same one rounding, so every reached entry that is
 *   neither NaN nor the identity has at least one winner.  (+0 and -0 compare equal.)
 *   Ties.  ties[s] is the number of winners of s, an exact integer.
 *   Weight.  Each winner of s carries w = G[s] / ties[s], divided once in the plan's type: the even split of
 *   torch.amin / torch.amax, which keeps the gradient mass of an entry equal to G[s].  G[s] is not read where
 *   ties[s] == 0.
 *   Gradient of mul.  Both _PLUS semirings: w goes to dAval[p] and to dBval[q].  MHS_SR_MAX_MIN (mul = min(a, b)):
 *   w goes to dAval[p] if a < b, to dBval[q] if b < a, and w / 2 to each if a == b (torch.minimum's rule).
 *   Duplicates and masks.  Every duplicate entry of A or B is a product of its own, as in the forward; a product
 *   outside a mask is no product.
 *   Outputs.  Every entry of a requested output is written; entries no winner reaches are exactly 0.
 *   Summation order.  dAval is summed without atomics in a fixed order: two calls give the same bits.  dBval is
 *   summed by atomics in any order.  For an output entry summed from m winning terms, with S the sum of their absolute
 *   values, the result is within (m + 1) u S of the exact sum of the exact weights, u = 2^-53 (FP64) or 2^-24 (FP32);
 *   the + 1 is the division's rounding.
 *   FP32.  An entry whose forward product or result was subnormal is exempt (the flush the forward documents).
 * ties holds nnz(C) device ints: the scratch of the tie count and an output of its own -- the number of optimal
 * intermediate vertices per entry.  Either of dAval and dBval may be NULL, not both.  Aval, Bval, Cval, dCval and ties
 * are always needed: the winner test reads both operands.  Outputs must not overlap inputs or each other.
 * The call queues, on the context's stream, one pre-step -- the zero fills of ties and of the requested outputs -- and
 * two passes of the plan's backward launch list (classes, LDS regions and grids are the plus-times backward's): pass 1
 * counts the winners into ties, pass 2 hands each winner's weight on.  ms and MHS_OPT_SYNC as in
 * mhs_spgemm_values_grad; with ms == NULL and MHS_OPT_SYNC 0 the call allocates nothing, reads nothing back and does
 * not synchronise.  Masked plans of all three forms are served.
 * Refused with MHS_ERR_INVALID and a message before any HIP call, writing nothing: a NULL ctx or plan, a needed array
 * NULL, both outputs NULL, a call of the wrong type, a plan of another device, and a MHS_SR_PLUS_TIMES plan -- the
 * message names the semiring and points at mhs_spgemm_values_grad.  The four backward entry points above keep
 * refusing semiring plans.  There is no batched form: semiring plans have width 1.
 * Cost on MI355X: DESIGN section 17.  Additions to ABI version 10, like the entries above. */
int mhs_spgemm_values_subgrad(mhs_ctx *ctx, mhs_values_plan *plan, const double *Aval, const double *Bval,
                              const double *Cval, const double *dCval, int32_t *ties,
                              double *dAval, double *dBval, double *ms);
int mhs_spgemm_values_subgrad_f32(mhs_ctx *ctx, mhs_values_plan *plan, const float *Aval, const float *Bval,
                                  const float *Cval, const float *dCval, int32_t *ties,
                                  float *dAval, float *dBval, double *ms);

/* ---- semiring witnesses: the arg of min-plus, max-plus and max-min plans ----------------------
 * For the same callers when the value is not enough: the predecessor on a shortest path, the Viterbi back-pointer,
 * the parent in a BFS tree.  On a plan of semiring MHS_SR_MIN_PLUS, _MAX_PLUS or _MAX_MIN, Cval is the forward result
 * for (Aval, Bval); a kept product (p, q, s) has A entry p, B entry q and C slot s, and its inner index k is the column
 * of p, which is the row of q.
 *   Winner.  The subgradient's rule (previous section), the same test in the same kernels: mul(Aval[p], Bval[q]) ==
 *   Cval[s] as values in the plan's type, and Cval[s] is not the identity of add.  A NaN never wins; +0 and -0 are
 *   equal.
 *   Witness.  wit[s] is the smallest inner index k among the winners of s, and -1 where s has no winner: an entry no
 *   product reaches, an entry equal to the identity ("no path"), a NaN Cval[s].
 *   Duplicates and masks.  Every duplicate entry of A or B is a product of its own, but duplicates share their k: the
 *   result does not depend on them.  A product outside a mask is no product.
 *   Consistency.  wit[s] >= 0 exactly where the subgradient's ties[s] >= 1.
 *   Outputs.  Every entry of wit is written.
 *   Determinism.  A minimum of integers: the result does not depend on order, and two calls give the same ints, on
 *   every class.
 *   FP32.  An entry whose forward product or result was subnormal is exempt (the flush the forward documents).
 * wit holds nnz(C) device ints and must not overlap the inputs.
 * The call queues, on the context's stream, one pre-step -- the fill of wit with -1 -- and one pass of the plan's
 * backward launch list, run by the subgradient's kernels as their third pass: every winner takes the minimum of its k
 * into wit[s].  ms and MHS_OPT_SYNC as in mhs_spgemm_values_subgrad; with ms == NULL and MHS_OPT_SYNC 0 the call
 * allocates nothing, reads nothing back and does not synchronise.  Masked plans of all three forms are served.
 * Refused with MHS_ERR_INVALID and a message before any HIP call, writing nothing: a NULL ctx or plan, a NULL Aval,
 * Bval, Cval or wit, a call of the wrong type, a plan of another device, and a MHS_SR_PLUS_TIMES plan -- the message
 * names the semiring and says that a sum has no witness.  There is no batched form: semiring plans have width 1.
 * Cost on MI355X: DESIGN section 18.  Additions to ABI version 10, like the entries above. */
int mhs_spgemm_values_witness(mhs_ctx *ctx, mhs_values_plan *plan, const double *Aval, const double *Bval,
                              const double *Cval, int32_t *wit, double *ms);
int mhs_spgemm_values_witness_f32(mhs_ctx *ctx, mhs_values_plan *plan, const float *Aval, const float *Bval,
                                  const float *Cval, int32_t *wit, double *ms);

/* ---- mixed-precision values plans: FP32 values summed in FP64 ---------------------------------
 * For float32 callers on patterns where LDS sums carry the call (many products per C entry): the LDS float add is far
 * slower than the double one on this chip, and an FP32 forward is then slower than the FP64 one.
 * A mixed plan takes float arrays and sums in double.  The sum type is a fifth fixed property of a plan, beside its
 * value type, its width, its mask form and its semiring:
 *   MHS_ACC_NATIVE   sums in the plan's value type: mhs_values_plan_create_accum is then exactly
 *                    mhs_values_plan_create_batched
 *   MHS_ACC_F64      with MHS_F64: the plain FP64 plan (mhs_values_plan_accum reports MHS_ACC_NATIVE);
 *                    with MHS_F32: the mixed plan
 * Any other accum returns MHS_ERR_INVALID before any HIP call, with a message naming the argument.  Mixed plans are
 * plus-times only (min and max are exact in any type: the semiring creation call has no such argument).
 * A mixed plan's classes, row lists, LDS needs and both launch plans are computed at the sum bytes 8 * width (width
 * 1, 2 or 4): mhs_values_plan_info shows the rows per class of the FP64 plan of the same patterns and width, and
 * mhs_values_plan_dtype says MHS_F32.  Validation, borrowing, plan memory, mhs_values_plan_kept, _width and _destroy
 * are those of any plan.
 * Hot calls are the existing _f32 entry points -- mhs_spgemm_values_f32, mhs_spgemm_values_batched_f32,
 * mhs_spgemm_values_grad_f32, mhs_spgemm_values_grad_batched_f32 -- the plan knows its sum type; a double call on a
 * mixed plan is refused as on any FP32 plan.  Stream, ms, MHS_OPT_SYNC and the contract of no allocation, no
 * read-back and no synchronise are unchanged.
 * The forward on a mixed plan.  On the team, wave, block and dot classes (rows[1..5] and rows[7]):
 *   each product is formed in double from the two floats, which is exact (24 + 24 bits <= 53);
 *   sums are double -- in LDS, in a register for the dot class;
 *   each entry is rounded to float once, at its store.
 *   For an entry of m kept products, E their exact sum and S the sum of their absolute values:
 *     |got - E| <= 2^-24 |E| + m * 2^-53 * S * (1 + 2^-24).
 *   Entries that no kept product reaches are exactly 0.0f.  Dot rows keep their fixed order, and their bits from call
 *   to call and inside any batch.
 * Global class (rows[6] of mhs_values_plan_info says how many rows this concerns): C's float segment stays the
 * accumulator -- the FP32 plan's kernel, float atomics, the FP32 bound m * 2^-24 * S.  There is no double scratch for
 * these rows.
 * Inf, NaN and stored zeros: products are classified in double on the exactly converted operands, and the data
 * contract's rule then gives NaN, +Inf or -Inf.  Otherwise the finite double sum is rounded to float once, and becomes
 * +-Inf only where it leaves the float range: a product of two finite floats that would overflow in float does not
 * poison its entry on its own (3e38 * 2 - 3e38 * 2 + 2^50 * 2^50 is exactly 2^100 here in any order, Inf or NaN on an
 * FP32 plan; with a third product of 1 the bound above still holds, but S is then 1.2e39 and 1 is below m 2^-53 S).  An
 * entry whose float rounding is subnormal is exempt, as on FP32 plans.
 * The backward on a mixed plan is the FP32 plan's, run on the launch list planned at 8 * width bytes: the float
 * kernels, float register sums for dAval in a fixed order, FP32 atomics for dBval, the FP32 bound.  The subgradient
 * and witness entry points keep refusing plus-times plans.
 * Cost on MI355X: on cant-like, where one LDS add per product carries the call, the mixed forward
 * takes 0.374 ms against the FP32 plan's 1.68 and the FP64 plan's 0.360 (the 4 % over FP64 is contention among the LDS
 * adds of the block-direct kernel, whose loads return sooner; not the conversions), and a width-2 batched call 0.76x the
 * FP64 one;
 * where loads and searches carry the call (scircuit-like, triangle) it is level with the FP32 plan at width 1 and, having
 * the FP64 classes, up to twice as slow at width 4: use it on LDS-bound patterns.
 * Additions to ABI version 10, like the entries above. */
typedef enum mhs_accum { MHS_ACC_NATIVE = 0, MHS_ACC_F64 = 1 } mhs_accum;
int mhs_values_plan_create_accum(mhs_ctx *ctx, const mhs_csr *A, const mhs_csr *B, const mhs_csr *C,
                                 int masked, int form, int dtype, int width, int accum, mhs_values_plan **plan);
/* The plan's sum type (mhs_accum): MHS_ACC_F64 on a mixed plan only. */
int mhs_values_plan_accum(const mhs_values_plan *plan, int *accum);

/* ---- soft semiring plans: log-sum-exp min-plus and max-plus, and their gradient ---------------
 * For the callers of the subgradient section when the product is the smoothed one: the forward algorithm of an HMM or
 * CRF, the inner step of soft-DTW, the soft-min relaxation of a shortest-path step.  Smoothing is a sixth fixed
 * property of a plan, beside its value type, width, mask form, semiring and sum type:
 *   MHS_SMOOTH_NONE   mhs_values_plan_create_smooth is then exactly mhs_values_plan_create_semiring
 *   MHS_SMOOTH_LSE    on MHS_SR_MIN_PLUS or MHS_SR_MAX_PLUS: the reduce is log-sum-exp at unit temperature
 * MHS_SMOOTH_LSE with MHS_SR_PLUS_TIMES, MHS_SR_MAX_MIN or any other semiring, and any other smooth, return
 * MHS_ERR_INVALID before any HIP call, with a message naming the argument.  The width is 1; masked plans of all three
 * forms are served.  mhs_values_plan_semiring reports the semiring that was smoothed, mhs_values_plan_smooth
 * MHS_SMOOTH_LSE on such a plan and MHS_SMOOTH_NONE on every other, mhs_values_plan_width 1.  A smoothed plan holds two
 * LDS planes per C entry, a running max and a sum: its classes, row lists, LDS needs and both launch plans are computed
 * at the sum bytes 2 * sizeof(value), so mhs_values_plan_info shows the rows per class of the width-2 plus-times plan
 * of the same patterns and type.
 * The forward runs through the existing hot calls -- mhs_spgemm_values, _f32, _batched, _batched_f32 (nb runs, as on any
 * width-1 plan); stream, ms, MHS_OPT_SYNC and the contract of no allocation, no read-back and no synchronise are
 * unchanged.  With v_k = fl(A(i,k) + B(k,j)), formed once in the plan's type, for the kept products of an entry:
 *   smoothed max-plus   C = M + log sum_k exp(v_k - M),        M  = max_k v_k
 *   smoothed min-plus   C = -(M' + log sum_k exp(-v_k - M')),   M' = max_k (-v_k)
 *   Unit temperature only: a caller with temperature tau scales the values by 1 / tau and the result by tau.
 *   Every duplicate entry of A or B is a product of its own, as on the hard plans; a product outside a mask is no
 *   product.  Every entry of the C segment is written.
 *   An entry that no kept product reaches, or all of whose products equal the identity of the hard semiring ("no edge"
 *   everywhere), gets that identity: +Inf (min-plus), -Inf (max-plus).  An identity product beside finite ones adds
 *   nothing.  A product equal to the opposite infinity makes the entry that infinity.  A NaN product leaves its entry
 *   either NaN or the result of its other products, and touches no other entry.
 *   An entry with one kept product has that product's bits.
 *   Bound.  u = 2^-53 (FP64) or 2^-24 (FP32), E the exact result on the v_k, m the kept products of the entry,
 *   V = max |v_k|; c_exp = 2 and c_log = 2 (FP64), c_exp = 2 and c_log = 4 (FP32): the worst error in ulps observed
 *   for the device's exp and log / log1p on 2^20 points each (0.88 and 0.64; 1.00 and 2.33), rounded up, plus 1
 *   (tools/ulp_probe.hip, profiles/smooth/ulp_probe.txt).
 *     team, wave, block and dot rows:   |got - E| <= 1.01 u (|E| + 2 m + 2 c_exp + 2 c_log ln m)
 *     global rows (rows[6] of mhs_values_plan_info says how many: the row's Cval segment is the accumulator, every
 *     product one compare-and-swap of max + log1p(exp(-|c - v|))):
 *                                       |got - E| <= 1.01 m u (V + ln m + 2 c_exp + 2 c_log + 1)
 *   Dot rows have a fixed order and the same bits on every call; the other classes sum by LDS atomics in any order.
 * The gradient, mhs_spgemm_values_softgrad, is the true gradient, in one pass; there are no ties.  Cval is the forward's
 * result for (Aval, Bval), handed in as for the subgradient, and G = dCval.  A kept product (p, q, s) carries
 *   w = G[s] * exp(v - Cval[s])   (max-plus)        w = G[s] * exp(Cval[s] - v)   (min-plus)
 * -- softmax weights: the marginals -- and the same w goes to dAval[p] and to dBval[q].  An entry whose Cval[s] is not
 * finite (identity, opposite infinity or NaN) passes nothing: exactly zero weights.  Either of dAval and dBval may be
 * NULL, not both; Aval, Bval, Cval and dCval are always needed.  Outputs must not overlap inputs or each other.  Every
 * entry of a requested output is written; entries no product reaches are exactly 0.  dAval is summed without atomics
 * in a fixed order: two calls give the same bits.  dBval is summed by atomics in any order.
 *   Bound.  For an output entry summed from m' terms w_k = G[s] exp(-+(v_k - Cval[s])), exact on the Cval handed in,
 *   with S = sum |w_k| and D = max |v_k - Cval[s]|:  |got - exact| <= 1.01 (m' + D + 2 c_exp + 1) u S; FP32 adds
 *   m' 2^-126 max |G|, because a subnormal weight may be flushed.
 * The call queues, on the context's stream, one pre-step -- the zero fills of the requested outputs -- and one pass of
 * the plan's backward launch list, the two planes holding G and Cval.  ms and MHS_OPT_SYNC as in
 * mhs_spgemm_values_grad; with ms == NULL and MHS_OPT_SYNC 0 the call allocates nothing, reads nothing back and does
 * not synchronise.
 * Refused with MHS_ERR_INVALID and a message before any HIP call, writing nothing: mhs_spgemm_values_softgrad on a plan
 * that is not smoothed (the message points at mhs_spgemm_values_subgrad or mhs_spgemm_values_grad); the subgradient and
 * the witness entry points on a smoothed plan (a soft reduce has weights, not winners, and no witness: the message
 * points at mhs_spgemm_values_softgrad); the four plus-times backward entry points, which refuse by semiring and name
 * mhs_spgemm_values_softgrad when the plan is smoothed; a call of the wrong type; a plan of another device; a NULL ctx,
 * plan or needed array; both outputs NULL.
 * Cost on MI355X.  The forward walks the pattern twice (max, then the sum of exp): 2.1x the hard
 * forward of the same semiring where loads and searches carry the call (scircuit-like: 0.455 against 0.217 ms in FP64),
 * 2.3-2.4x on a masked triangle, and more than expected where LDS atomics carry it -- cant-like: 1.19 against 0.358 ms in
 * FP64 (3.3x: one double exp per product beside the add) and 1.96 against 0.244 ms in FP32 (8.0x: the second walk's
 * reduce is the slow LDS float add, which the hard FP32 plan never issues); on such patterns prefer an FP64 plan.  The
 * gradient is one pass where the subgradient makes two: 0.24-0.26x the subgradient call for dAval alone, 0.46-0.77x for
 * dBval or both, and 1.0-1.3x the plus-times backward of the same pattern and type (dAval alone: 1.1-2.0x).
 * Additions to ABI version 10, like the entries above. */
typedef enum mhs_smooth { MHS_SMOOTH_NONE = 0, MHS_SMOOTH_LSE = 1 } mhs_smooth;
int mhs_values_plan_create_smooth(mhs_ctx *ctx, const mhs_csr *A, const mhs_csr *B, const mhs_csr *C,
                                  int masked, int form, int dtype, int semiring, int smooth, mhs_values_plan **plan);
/* Whether the plan is smoothed (mhs_smooth). */
int mhs_values_plan_smooth(const mhs_values_plan *plan, int *smooth);
int mhs_spgemm_values_softgrad(mhs_ctx *ctx, mhs_values_plan *plan, const double *Aval, const double *Bval,
                               const double *Cval, const double *dCval, double *dAval, double *dBval, double *ms);
int mhs_spgemm_values_softgrad_f32(mhs_ctx *ctx, mhs_values_plan *plan, const float *Aval, const float *Bval,
                                   const float *Cval, const float *dCval, float *dAval, float *dBval, double *ms);

/* At = A^T on the device (the reference's AAT operand: B = transpose(A),
 * src/main.cu:98-99 with AAT=1, inc/common.h:37; host transpose src/utils.cpp:20-46).
 * At->M = A->N, At->N = A->M; rows of At list their columns ascending; arrays are
 * fresh device allocations owned by the caller (mhs_csr_free).  Synchronous. */
int mhs_transpose(mhs_ctx *ctx, const mhs_csr *A, mhs_csr *At);

/* Free a device CSR produced by mhs_spgemm (hipFree) and zero the struct. */
void mhs_csr_free(mhs_csr *C);
/* Return C's device buffers to ctx's output pool for reuse by later calls
 * (a caching allocator: avoids hipMalloc/hipFree per call). */
void mhs_ctx_recycle(mhs_ctx *ctx, mhs_csr *C);

/* ---- host-side helpers (the reference's L1 layer) ---------------------- */

/* Host CSR (malloc'ed arrays). */
typedef struct mhs_host_csr {
    int32_t M, N, nnz;
    int32_t *ptr, *col;
    double *val;
    int32_t is_symmetric;
} mhs_host_csr;

/* readMtxFile (inc/mmio_read.h:34-159): real/integer/pattern(1.0)/complex
 * (real part); symmetric and hermitian off-diagonals mirrored, skew not;
 * duplicates kept; rows sorted by (col, val).  Returns MHS_OK or MHS_ERR_IO. */
int mhs_read_mtx(const char *path, mhs_host_csr *A);
void mhs_host_csr_free(mhs_host_csr *A);
/* Binary CSR cache (replaces re-running the fscanf loop of
 * inc/mmio_read.h:80-108 on every run).  mhs_read_mtx_cached reads `cache_path`
 * (NULL: path + ".mhscsr") when its stamp matches the .mtx's size and mtime,
 * else parses the text with mhs_read_mtx and writes the cache (best effort);
 * *from_cache (may be NULL) says which.  The cache reader checks ptr/col
 * invariants and returns MHS_ERR_IO on a truncated or corrupt file. */
int mhs_read_mtx_cached(const char *path, const char *cache_path, mhs_host_csr *A, int *from_cache);
int mhs_write_csr_bin(const char *path, const mhs_host_csr *A, int64_t src_size, int64_t src_mtime_ns);
int mhs_read_csr_bin(const char *path, mhs_host_csr *A, int64_t *src_size, int64_t *src_mtime_ns);
/* int_result of src/main.cu:102-107. */
uint64_t mhs_flop_count(int32_t nnzA, const int32_t *Acol, const int32_t *Bptr);

/* Device memory helpers for callers without their own HIP runtime binding
 * (e.g. ctypes).  kind: 0 = H2D, 1 = D2H, 2 = D2D.  Synchronous on ctx's stream. */
int mhs_memcpy(mhs_ctx *ctx, void *dst, const void *src, size_t bytes, int kind);
int mhs_device_alloc(mhs_ctx *ctx, void **p, size_t bytes);
int mhs_device_free(mhs_ctx *ctx, void *p);

/* Measured HBM bandwidth of the context's device (a diagnostic beside the 8 TB/s spec that
 * the roofline fractions are priced against; not on the SpGEMM path): streaming kernels over
 * two `bytes` buffers (>= 1 MiB; allocated and freed inside), each run `iters` times
 * between hipEvents.  gbps[0] = copy (read + write bytes), gbps[1] = read, gbps[2] = write,
 * in GB/s (1e9 B/s).  Synchronous. */
int mhs_hbm_peak(mhs_ctx *ctx, size_t bytes, int iters, double *gbps);

int mhs_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* MHSPGEMM_H */
