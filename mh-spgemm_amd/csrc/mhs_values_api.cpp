// mhs_values_api.cpp -- the C ABI of the values-only SpGEMM (include/mhspgemm.h): values plans on a
// kept or masked pattern, the values call and its backward.
//
// Plan creation (values_plan_create) is the only part with host round trips; it runs as numbered steps
//   1 the three row_ptr arrays -> 2 A's and C's columns -> 3 classify and verify (3m, a mask: B's
//   columns, B^T, classify, count the kept products) -> one read-back of counters and status
// on the context's stream, each check read back before the next step indexes through what it checked.
// A hot call (mhs_spgemm_values, mhs_spgemm_values_grad and their _f32 forms) is its argument checks and
// run_values: the plan's launch list issued on the context's stream, timed by the plan's event pair when asked.
// A plan has one value type (mhs_dtype), fixed at creation: its classes, lists and launch plans are computed
// for that type's size, and a call of the other type is refused before any HIP call.
// A plan also has a width (mhs_values_plan_create_batched: 1, 2 or 4 value sets per walk), fixed likewise: it
// classifies at the sum bytes width x size.  Every forward call is spgemm_values_batched: ceil(nb / width)
// passes of the launch list inside the one run_values frame; the unbatched entry points are its nb = 1.  The
// batched backward (mhs_spgemm_values_grad_batched) makes the same passes over the backward's launch list.
// A plan has a semiring too (mhs_values_plan_create_semiring; mhs_semiring.hpp), fixed likewise: classes and launch
// plans do not depend on it, the forward's issue passes it on to the kernels' policy, and the backward entry points
// refuse a plan of another semiring than plus-times (check_grad_semiring).  Such a plan's backward is its subgradient
// (spgemm_values_subgrad): two passes of the backward's launch list, which in turn refuses a plus-times plan.  Its
// witness (spgemm_values_witness) is a third pass of the same kernels on a call of its own: the smallest inner index
// among the winners of every C entry.
// A plan has a sum type as well (mhs_values_plan_create_accum; ValAccum), fixed likewise: a mixed plan -- FP32 values,
// FP64 sums -- classifies at width x 8 where its values are 4 bytes; its forward's issue passes the sum type on to
// the kernels, and its backward is the float kernels on the launch list planned at those bytes.
// A plan may be smoothed (mhs_values_plan_create_smooth; mhs_smooth.hpp), fixed likewise: a min-plus or max-plus plan
// whose reduce is log-sum-exp.  It classifies at twice its value's bytes -- a max plane and a sum plane per C entry --
// at width 1; the forward's issue sends it to the smoothed kernels, its backward is its gradient
// (spgemm_values_softgrad: one pass of the backward's launch list), and the subgradient and the witness refuse it.
// Kernels and launchers: mhs_values.hip, mhs_values_grad.hip, mhs_values_subgrad.hip, mhs_values_smooth.hip (declared in mhs_valwalk.hpp); classes,
// launch plans, counter block and status words: mhs_valplan.hpp.
#include "mhs_ctx.hpp"
#include "mhs_smooth.hpp"
#include "mhs_valwalk.hpp"

#include <cstdlib>
#include <memory>

using namespace mhs;

// A values plan (mhs_values_plan_create): the six borrowed pattern arrays, the class lists and the
// launch plan.  Its device memory is its own (not the context workspace): mhs_spgemm calls and
// mhs_ctx_trim on the same context leave it alone.
struct mhs_values_plan {
    int device = 0;
    int dtype = MHS_F64;    // mhs_dtype: the type of every value array of its calls
    int width = 1;          // value sets a walk of its forward kernels sums (1, 2 or 4)
    int semiring = SR_PLUS_TIMES;  // mhs_semiring: what its forward kernels reduce the kept products with
    int accum = VAL_ACC_NATIVE;    // mhs_accum: VAL_ACC_F64 on a mixed plan (dtype MHS_F32, sums in FP64) only
    int smooth = SMOOTH_NONE;      // mhs_smooth: SMOOTH_LSE on a min-plus or max-plus plan whose reduce is log-sum-exp
    ValPattern pat{};
    long long nnzA = 0, nnzB = 0, nnzC = 0, products = 0;
    long long kept = 0;    // products that land in C's pattern (masked plans count them; else = products)
    char* mem = nullptr;   // lists (M ints), counters (VAL_CNT_INTS), status (VAL_STATUS_INTS)
    size_t mem_bytes = 0;
    // a masked plan with dot rows: B^T's pattern -- tptr (B.N + 1), trow, tperm (nnz(B) each) -- the plan's own too
    char* tmem = nullptr;
    size_t tmem_bytes = 0;
    ValTrans trans{};
    int* lists = nullptr;
    int list_off[VAL_NCLASS] = {};
    ValCounts counts{};
    ValPlan plan{};
    ValPlan gplan{};        // the backward's launches (plan_grad)
    hipEvent_t ev[2] = {};  // timed calls
};

namespace {

constexpr int dtype_bytes(int dtype) { return dtype == MHS_F32 ? VAL_VB_F32 : VAL_VB_F64; }
// The bytes a plan classifies at: its width x the size of its sums (a mixed plan's: 8, its value's 4); a smoothed
// plan's two planes stand where a width-2 plan's two sums do
int sum_bytes(const mhs_values_plan* p) {
    return val_sum_bytes(dtype_bytes(p->dtype), p->width * val_smooth_planes(p->smooth), p->accum);
}
static_assert((int)MHS_SMOOTH_NONE == (int)SMOOTH_NONE && (int)MHS_SMOOTH_LSE == (int)SMOOTH_LSE, "mhs_smooth is ValSmooth");
static_assert(MHS_VAL_WIDTH_MAX == VAL_WIDTH_MAX, "the header's width is the plan's");
static_assert((int)MHS_ACC_NATIVE == (int)VAL_ACC_NATIVE && (int)MHS_ACC_F64 == (int)VAL_ACC_F64, "mhs_accum is ValAccum");
const char* dtype_name(int dtype) { return dtype == MHS_F32 ? "FP32" : "FP64"; }
// ... of a plan: its value type, and its sum type where that is another
const char* plan_type_name(const mhs_values_plan* p) { return p->accum == VAL_ACC_F64 ? "FP32, FP64 sums" : dtype_name(p->dtype); }
template <class V>
constexpr int dtype_of() {
    static_assert(sizeof(V) == VAL_VB_F64 || sizeof(V) == VAL_VB_F32, "double or float");
    return sizeof(V) == VAL_VB_F32 ? MHS_F32 : MHS_F64;
}

static_assert((int)MHS_SR_PLUS_TIMES == (int)SR_PLUS_TIMES && (int)MHS_SR_MIN_PLUS == (int)SR_MIN_PLUS &&
                  (int)MHS_SR_MAX_PLUS == (int)SR_MAX_PLUS && (int)MHS_SR_MAX_MIN == (int)SR_MAX_MIN,
              "mhs_semiring is ValSemiring");
static_assert((int)MHS_MASK_AUTO == (int)VM_AUTO && (int)MHS_MASK_PRODUCT == (int)VM_PRODUCT && (int)MHS_MASK_DOT == (int)VM_DOT,
              "mhs_mask_form is ValMaskForm");

// AUTO's ratio: VAL_DOT_RATIO, or MHS_VAL_DOT_RATIO (diagnostic: one build swept over the ratio)
int val_dot_ratio() {
    if (const char* v = std::getenv("MHS_VAL_DOT_RATIO")) {
        const long r = std::strtol(v, nullptr, 10);
        if (r >= 1 && r <= 1 << 20) return (int)r;
    }
    return VAL_DOT_RATIO;
}

// Device scratch with one owner: freed once, when the owner goes -- in plan creation after the stream
// that used it has been read back (or synchronized by the failed plan's destruction).
struct HipFree {
    void operator()(void* p) const { (void)hipFree(p); }
};
using Scratch = std::unique_ptr<void, HipFree>;

// A plan under construction: the steps of values_plan_create.  Each returns MHS_OK or the call's error
// (message set); the plan is the caller's to destroy.
struct PlanBuild {
    mhs_ctx* ctx;
    mhs_values_plan* p;
    const mhs_csr *A, *B, *C;
    hipStream_t s;
    int *d_cnt = nullptr, *d_status = nullptr;
    int status[VAL_STATUS_INTS];
    int h_cnt[VAL_CNT_INTS];
    static constexpr int NONE = 0x7f7f7f7f;  // a status word's fill: any row index is below it, as below INT_MAX

    int hip(hipError_t e, const char* what) const { return e == hipSuccess ? MHS_OK : fail_hip(ctx, e, what); }
    // the status words on the host, once the stream has run what was launched
    int read_status(const char* what) {
        hipError_t r = hipGetLastError();
        if (r == hipSuccess) r = hipMemcpyAsync(status, d_status, sizeof status, hipMemcpyDeviceToHost, s);
        if (r == hipSuccess) r = hipStreamSynchronize(s);
        return hip(r, what);
    }
    int bad_row(int k, const char* what) const {
        if (status[k] == NONE) return MHS_OK;
        return fail(ctx, MHS_ERR_INVALID,
                    std::string("mhs_values_plan_create: ") + what + " (first at row " + std::to_string(status[k]) + ")");
    }

    // 0. the plan's own memory: lists, counter block (zero), status words (NONE), and its event pair
    int allocate() {
        const size_t lists_bytes = al((size_t)(A->M > 0 ? A->M : 1) * 4);
        p->mem_bytes = lists_bytes + al((size_t)VAL_CNT_INTS * 4) + al((size_t)VAL_STATUS_INTS * 4);
        if (const int rc = hip(hipMalloc((void**)&p->mem, p->mem_bytes), "mhs_values_plan_create: plan memory")) return rc;
        if (const int rc = hip(poison_fill(ctx, p->mem, p->mem_bytes, s), "plan memory (MHS_POISON)")) return rc;
        for (hipEvent_t& ev : p->ev)
            if (const int rc = hip(hipEventCreate(&ev), "mhs_values_plan_create: events")) return rc;
        p->lists = (int*)p->mem;
        d_cnt = (int*)(p->mem + lists_bytes);
        d_status = d_cnt + al((size_t)VAL_CNT_INTS * 4) / 4;
        if (const int rc = hip(hipMemsetAsync(d_cnt, 0, (size_t)VAL_CNT_INTS * 4, s), "plan counters")) return rc;
        return hip(hipMemsetAsync(d_status, 0x7f, (size_t)VAL_STATUS_INTS * 4, s), "plan status");
    }
    // 1. the three row_ptr arrays: everything after this indexes through them
    int check_row_ptr() {
        launch_val_check_ptr(A->ptr, A->M, A->nnz, d_status + VS_APTR, s);
        launch_val_check_ptr(B->ptr, B->M, B->nnz, d_status + VS_BPTR, s);
        launch_val_check_ptr(C->ptr, C->M, C->nnz, d_status + VS_CPTR, s);
        if (const int rc = read_status("mhs_values_plan_create: row_ptr check")) return rc;
        if (const int rc = bad_row(VS_APTR, "A.ptr is not a row_ptr of nnz(A) entries")) return rc;
        if (const int rc = bad_row(VS_BPTR, "B.ptr is not a row_ptr of nnz(B) entries")) return rc;
        if (const int rc = bad_row(VS_CPTR, "C.ptr is not monotone from 0 to C.nnz")) return rc;
        if ((A->M == 0 && A->nnz != 0) || (B->M == 0 && B->nnz != 0) || (C->M == 0 && C->nnz != 0))
            return fail(ctx, MHS_ERR_INVALID, "mhs_values_plan_create: entries without rows");
        return MHS_OK;
    }
    // 2. A's columns index B's rows; C's columns ascend strictly within [0, C.N)
    int check_columns() {
        launch_val_check_cols(A->ptr, A->col, A->M, B->M, false, d_status + VS_ACOL, s);
        launch_val_check_cols(C->ptr, C->col, C->M, C->N, true, d_status + VS_CCOL, s);
        if (const int rc = read_status("mhs_values_plan_create: column check")) return rc;
        if (const int rc = bad_row(VS_ACOL, "a column of A is outside [0, B.M)")) return rc;
        return bad_row(VS_CCOL, "C's columns are not strictly ascending within [0, C.N)");
    }
    // 3. classes, lists, and every product's column looked up in its C row
    void classify_and_verify() {
        launch_val_classify(p->pat, sum_bytes(p), d_cnt, p->lists, s);
        launch_val_verify(p->pat, d_status + VS_PRODUCTS, s);
    }
    // 3m. a mask: B^T's pattern for the dot class (its sort indexes by B's columns: checked first; its scratch
    // is sort_tmp's), classes by val_class_masked, and the products that land in the mask counted where the
    // plain plan verifies
    int classify_and_count(int form, Scratch& sort_tmp) {
        if (form != MHS_MASK_PRODUCT) {
            launch_val_check_cols(B->ptr, B->col, B->M, B->N, false, d_status + VS_BCOL, s);
            if (const int rc = read_status("mhs_values_plan_create: column check")) return rc;
            if (const int rc = bad_row(VS_BCOL, "a column of B is outside [0, B.N)")) return rc;
            const Csr b{B->M, B->N, B->nnz, B->ptr, B->col, nullptr};
            const size_t nb = (size_t)B->nnz;
            const size_t ptr_bytes = al(((size_t)B->N + 1) * 4), ent_bytes = al((nb ? nb : 1) * 4);
            size_t tmp_bytes = 0;
            if (const int rc = hip(transpose_pattern(b, nullptr, nullptr, nullptr, nullptr, &tmp_bytes, s),
                                   "mhs_values_plan_create: B^T (scratch size)"))
                return rc;
            if (const int rc = hip(hipMalloc((void**)&p->tmem, ptr_bytes + 2 * ent_bytes), "mhs_values_plan_create: B^T memory"))
                return rc;
            p->tmem_bytes = ptr_bytes + 2 * ent_bytes;
            if (const int rc = hip(poison_fill(ctx, p->tmem, p->tmem_bytes, s), "B^T memory (MHS_POISON)")) return rc;
            int* tptr = (int*)p->tmem;
            int* trow = (int*)(p->tmem + ptr_bytes);
            int* tperm = (int*)(p->tmem + ptr_bytes + ent_bytes);
            void* tmp = nullptr;
            hipError_t e = hipMalloc(&tmp, tmp_bytes ? tmp_bytes : 16);
            sort_tmp.reset(tmp);
            if (e == hipSuccess) e = poison_fill(ctx, tmp, tmp_bytes ? tmp_bytes : 16, s);
            if (e == hipSuccess) e = transpose_pattern(b, tptr, trow, tperm, tmp, &tmp_bytes, s);
            if (const int rc = hip(e, "mhs_values_plan_create: B^T")) return rc;
            p->trans = ValTrans{tptr, trow, tperm};
        }
        launch_val_classify_masked(p->pat, ValMask{p->trans.tptr, form, val_dot_ratio()}, sum_bytes(p), d_cnt, p->lists, s);
        launch_val_count_kept(p->pat, d_cnt, s);
        return MHS_OK;
    }
    // The one read-back of step 3: the counter block and the status words, then the launch plans from them
    int read_back(bool masked) {
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(h_cnt, d_cnt, sizeof h_cnt, hipMemcpyDeviceToHost, s);
        if (const int rc = hip(e, "mhs_values_plan_create: classify")) return rc;
        if (const int rc = read_status("mhs_values_plan_create: classify")) return rc;
        if (!masked)
            if (const int rc = bad_row(VS_PRODUCTS, "C's pattern misses a column of the product A*B")) return rc;
        int off = 0;
        for (int c = 0; c < VAL_NCLASS; ++c) {
            p->counts.rows[c] = h_cnt[val_cnt_rows(c)];
            p->counts.need[c] = h_cnt[val_cnt_need(c)];
            p->list_off[c] = off;
            off += p->counts.rows[c];
        }
        memcpy(&p->products, &h_cnt[VAL_CNT_PRODUCTS], sizeof p->products);
        p->kept = p->products;
        if (masked) memcpy(&p->kept, &h_cnt[VAL_CNT_KEPT], sizeof p->kept);
        if (p->tmem && p->counts.rows[VC_DOT] == 0) {  // no row chose the dot class: B^T goes again
            (void)hipFree(p->tmem);
            p->tmem = nullptr;
            p->tmem_bytes = 0;
            p->trans = ValTrans{};
        }
        p->plan = plan_values(p->counts, sum_bytes(p));
        p->gplan = plan_grad(p->counts, sum_bytes(p));  // (a wide plan's serves mhs_spgemm_values_grad_batched)
        return MHS_OK;
    }
};

// mhs_values_plan_create (masked false: C must contain the product's pattern) and
// mhs_values_plan_create_masked (C is a mask; form: mhs_mask_form), for values of `dtype` (mhs_dtype).
// width: the value sets a walk sums (mhs_values_plan_create_batched; 1 for every other entry point).
// semiring: mhs_semiring (mhs_values_plan_create_semiring; MHS_SR_PLUS_TIMES for every other entry point); another
// one than plus-times has width 1.
// accum: mhs_accum (mhs_values_plan_create_accum; MHS_ACC_NATIVE for every other entry point); MHS_ACC_F64 on MHS_F64
// is the native plan, on MHS_F32 the mixed one, which is plus-times.
// smooth: mhs_smooth (mhs_values_plan_create_smooth; MHS_SMOOTH_NONE for every other entry point); MHS_SMOOTH_LSE needs
// min-plus or max-plus.
int values_plan_create(mhs_ctx* ctx, const mhs_csr* A, const mhs_csr* B, const mhs_csr* C, bool masked, int form, int dtype,
                       int width, int semiring, int accum, int smooth, mhs_values_plan** out) {
    if (!ctx) return MHS_ERR_INVALID;
    if (!A || !B || !C || !out) return fail(ctx, MHS_ERR_INVALID, "mhs_values_plan_create: null argument");
    *out = nullptr;
    if (!val_smooth_ok(smooth))
        return fail(ctx, MHS_ERR_INVALID,
                    "mhs_values_plan_create: smooth " + std::to_string(smooth) + " is not an mhs_smooth (MHS_SMOOTH_NONE or MHS_SMOOTH_LSE)");
    if (smooth != SMOOTH_NONE && !val_smooth_serves(semiring))
        return fail(ctx, MHS_ERR_INVALID,
                    "mhs_values_plan_create: smooth MHS_SMOOTH_LSE needs the semiring min_plus or max_plus, not " +
                        (val_semiring_ok(semiring) ? std::string(val_semiring_name(semiring)) : "semiring " + std::to_string(semiring)));
    if (!val_semiring_ok(semiring))
        return fail(ctx, MHS_ERR_INVALID,
                    "mhs_values_plan_create: semiring " + std::to_string(semiring) + " is not an mhs_semiring (0 to 3)");
    if (semiring != SR_PLUS_TIMES && width != 1)
        return fail(ctx, MHS_ERR_INVALID,
                    std::string("mhs_values_plan_create: a ") + val_semiring_name(semiring) + " plan has width 1");
    if (dtype != MHS_F64 && dtype != MHS_F32)
        return fail(ctx, MHS_ERR_INVALID, "mhs_values_plan_create: dtype is not an mhs_dtype (MHS_F64 or MHS_F32)");
    if (!val_accum_ok(accum))
        return fail(ctx, MHS_ERR_INVALID,
                    "mhs_values_plan_create: accum " + std::to_string(accum) + " is not an mhs_accum (MHS_ACC_NATIVE or MHS_ACC_F64)");
    if (dtype == MHS_F64) accum = VAL_ACC_NATIVE;  // (FP64 sums of FP64 values: the plain plan)
    if (accum == VAL_ACC_F64 && semiring != SR_PLUS_TIMES)
        return fail(ctx, MHS_ERR_INVALID,
                    std::string("mhs_values_plan_create: a plan of FP32 values and FP64 sums is plus_times only, not ") +
                        val_semiring_name(semiring));
    if (!val_width_ok(width))
        return fail(ctx, MHS_ERR_INVALID, "mhs_values_plan_create: width " + std::to_string(width) + " is not 1, 2 or 4");
    if (masked && (form < MHS_MASK_AUTO || form > MHS_MASK_DOT))
        return fail(ctx, MHS_ERR_INVALID, "mhs_values_plan_create: form is not an mhs_mask_form");
    if (A->M < 0 || A->N < 0 || A->nnz < 0 || B->M < 0 || B->N < 0 || B->nnz < 0 || C->M < 0 || C->N < 0 || C->nnz < 0)
        return fail(ctx, MHS_ERR_INVALID, "mhs_values_plan_create: negative dimension");
    if (A->N != B->M) return fail(ctx, MHS_ERR_INVALID, "mhs_values_plan_create: A.N != B.M");
    if (C->M != A->M) return fail(ctx, MHS_ERR_INVALID, "mhs_values_plan_create: C.M != A.M");
    if (C->N != B->N) return fail(ctx, MHS_ERR_INVALID, "mhs_values_plan_create: C.N != B.N");
    if ((A->M > 0 && (!A->ptr || !C->ptr)) || (B->M > 0 && !B->ptr) || (A->nnz > 0 && !A->col) || (B->nnz > 0 && !B->col) ||
        (C->nnz > 0 && !C->col))
        return fail(ctx, MHS_ERR_INVALID, "mhs_values_plan_create: null device array");
    MHS_HIP(hipSetDevice(ctx->device));
    mhs_values_plan* p = new mhs_values_plan();
    p->device = ctx->device;
    p->dtype = dtype;
    p->width = width;
    p->semiring = semiring;
    p->accum = accum;
    p->smooth = smooth;
    p->pat = ValPattern{A->M, A->ptr, A->col, B->ptr, B->col, C->ptr, C->col};
    p->nnzA = A->nnz, p->nnzB = B->nnz, p->nnzC = C->nnz;
    Scratch sort_tmp;  // (B^T's sort scratch: it outlives the build's last step, which syncs the stream either way)
    PlanBuild b{ctx, p, A, B, C, ctx->stream};
    int rc = b.allocate();
    if (rc == MHS_OK) rc = b.check_row_ptr();
    if (rc == MHS_OK) rc = b.check_columns();
    if (rc == MHS_OK && masked) rc = b.classify_and_count(form, sort_tmp);
    if (rc == MHS_OK && !masked) b.classify_and_verify();
    if (rc == MHS_OK) rc = b.read_back(masked);
    if (rc != MHS_OK) {
        mhs_values_plan_destroy(ctx, p);  // (synchronizes the stream: what it still runs may read the plan's memory)
        return rc;
    }
    *out = p;
    return MHS_OK;
}

// A values launch list on the context's stream: pre (the backward's zero fills; may be null) and then
// issue(launch) for each launch of `plan`, between the plan's events when ms is asked for (the call then
// returns with the launches done and their time), else followed by the context's sync if it is on.
template <class Pre, class Issue>
int run_values(mhs_ctx* ctx, mhs_values_plan* p, const ValPlan& plan, double* ms, Pre pre, Issue issue) {
    MHS_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    if (ms) MHS_HIP(hipEventRecord(p->ev[0], s));
    if (const int rc = pre(s)) return rc;
    for (int i = 0; i < plan.n; ++i) {
        const ValLaunch& l = plan.launch[i];
        issue(l, p->lists + p->list_off[l.cls], s);
    }
    MHS_HIP(hipGetLastError());
    if (ms) {
        float f = 0;
        MHS_HIP(hipEventRecord(p->ev[1], s));
        MHS_HIP(hipEventSynchronize(p->ev[1]));
        MHS_HIP(hipEventElapsedTime(&f, p->ev[0], p->ev[1]));
        *ms = f;
    } else if (ctx->sync) {
        MHS_HIP(hipStreamSynchronize(s));
    }
    return MHS_OK;
}

// Whether a call on values of V may run on the plan: its type is the plan's
template <class V>
int check_dtype(mhs_ctx* ctx, const mhs_values_plan* p, const char* call) {
    if (p->dtype == dtype_of<V>()) return MHS_OK;
    return fail(ctx, MHS_ERR_INVALID,
                std::string(call) + ": the plan's values are " + plan_type_name(p) + ", the call's " + dtype_name(dtype_of<V>()) +
                    " (the value type is fixed at plan creation: mhs_values_plan_create_typed)");
}

// Every forward call: mhs_spgemm_values_batched / _f32, and mhs_spgemm_values / _f32 as its nb = 1.  Set b reads
// Aval + b * sA and Bval + b * sB and writes Cval + b * sC.  The plan's launch list runs once per pass of up to
// `width` sets; pass q starts at set q * width, and the last one has the sets that remain.
template <class V>
int spgemm_values_batched(mhs_ctx* ctx, mhs_values_plan* p, int nb, const V* Aval, long long sA, const V* Bval, long long sB,
                          V* Cval, long long sC, double* ms, const char* call) {
    if (!ctx) return MHS_ERR_INVALID;
    if (!p) return fail(ctx, MHS_ERR_INVALID, std::string(call) + ": null plan");
    if (const int rc = check_dtype<V>(ctx, p, call)) return rc;
    if (nb < 1) return fail(ctx, MHS_ERR_INVALID, std::string(call) + ": nb = " + std::to_string(nb) + " (at least one value set)");
    if (sA < 0 || sB < 0 || sC < 0) return fail(ctx, MHS_ERR_INVALID, std::string(call) + ": negative stride");
    if ((sA > 0 && sA < p->nnzA) || (sB > 0 && sB < p->nnzB))
        return fail(ctx, MHS_ERR_INVALID,
                    std::string(call) + ": an input stride is 0 (one array shared by all sets) or at least the matrix's nnz");
    if (nb > 1 && sC < p->nnzC)
        return fail(ctx, MHS_ERR_INVALID, std::string(call) + ": strideC is below nnz(C): the sets' outputs would overlap");
    if ((p->nnzA > 0 && !Aval) || (p->nnzB > 0 && !Bval) || (p->nnzC > 0 && !Cval))
        return fail(ctx, MHS_ERR_INVALID, std::string(call) + ": null value array");
    if (p->device != ctx->device) return fail(ctx, MHS_ERR_INVALID, std::string(call) + ": the plan belongs to another device");
    const int W = p->width, passes = (nb + W - 1) / W;
    return run_values(
        ctx, p, p->plan, ms, [](hipStream_t) { return MHS_OK; },
        [&](const ValLaunch& l, const int* list, hipStream_t s) {
            for (int q = 0; q < passes; ++q) {
                const long long b = (long long)q * W;
                ValArgs<V> a{{p->pat.Aptr, p->pat.Acol, Aval + b * sA}, {p->pat.Bptr, p->pat.Bcol, Bval + b * sB},
                             {p->pat.Cptr, p->pat.Ccol, Cval + b * sC}};
                a.sA = sA, a.sB = sB, a.sC = sC;
                a.nw = nb - b < W ? (int)(nb - b) : W;
                if (p->smooth == SMOOTH_LSE) issue_values_smooth(l, p->semiring, a, p->trans, list, s);  // (W = 1)
                else issue_values(l, W, p->semiring, p->accum, a, p->trans, list, s);
            }
        });
}

// Whether the unbatched backward entry points may run on the plan: they serve width 1 only (a plan of any width
// has mhs_spgemm_values_grad_batched)
int check_grad_width(mhs_ctx* ctx, const mhs_values_plan* p, const char* call) {
    if (p->width == 1) return MHS_OK;
    return fail(ctx, MHS_ERR_INVALID,
                std::string(call) + ": the backward of batched plans is not built (the plan's width is " + std::to_string(p->width) +
                    "): a width-1 plan has to be used");
}

// Whether a backward entry point may run on the plan: min and max have subgradients only (spgemm_values_subgrad)
int check_grad_semiring(mhs_ctx* ctx, const mhs_values_plan* p, const char* call) {
    if (p->semiring == SR_PLUS_TIMES) return MHS_OK;
    return fail(ctx, MHS_ERR_INVALID,
                std::string(call) + ": the plan's semiring is " + val_semiring_name(p->semiring) +
                    ": the backward is built for plus_times plans only" +
                    (p->smooth == SMOOTH_LSE ? " (a smoothed plan's gradient is mhs_spgemm_values_softgrad)" : ""));
}

// Whether the subgradient or the witness may run on the plan: a smoothed plan would pass their semiring check
int check_hard_reduce(mhs_ctx* ctx, const mhs_values_plan* p, const char* call, const char* what) {
    if (p->smooth == SMOOTH_NONE) return MHS_OK;
    return fail(ctx, MHS_ERR_INVALID,
                std::string(call) + ": the plan is smoothed (MHS_SMOOTH_LSE on " + val_semiring_name(p->semiring) +
                    "): a soft reduce has weights, not winners, and " + what + ": its gradient is mhs_spgemm_values_softgrad");
}

// Zero fill of nb segments of n values, `stride` elements apart, as one call: a plain fill where the segments
// are contiguous (or there is one), a 2-D fill -- rows of n values at a pitch of `stride` -- where padding lies
// between them, which keeps its bytes.
template <class V>
hipError_t zero_sets(V* dst, long long n, long long stride, int nb, hipStream_t s) {
    if (!dst || n <= 0) return hipSuccess;
    if (nb == 1 || stride == n) return hipMemsetAsync(dst, 0, sizeof(V) * (size_t)n * (size_t)nb, s);
    return hipMemset2DAsync(dst, sizeof(V) * (size_t)stride, 0, sizeof(V) * (size_t)n, (size_t)nb, s);
}

// The zero fill of a backward's wanted outputs, nb sets of each (1: the unbatched calls): dB is summed into; dA is
// stored once per entry of a listed row, and rows without C entries are in no list.  One fill call per side.
template <class V>
hipError_t zero_grads(const mhs_values_plan* p, V* dAval, long long sDA, V* dBval, long long sDB, int nb, hipStream_t s) {
    const hipError_t e = zero_sets(dAval, p->nnzA, sDA, nb, s);
    return e == hipSuccess ? zero_sets(dBval, p->nnzB, sDB, nb, s) : e;
}

// mhs_spgemm_values_grad and mhs_spgemm_values_grad_f32
template <class V>
int spgemm_values_grad(mhs_ctx* ctx, mhs_values_plan* p, const V* Aval, const V* Bval, const V* dCval, V* dAval, V* dBval,
                       double* ms, const char* call) {
    if (!ctx) return MHS_ERR_INVALID;
    if (!p) return fail(ctx, MHS_ERR_INVALID, std::string(call) + ": null plan");
    if (const int rc = check_dtype<V>(ctx, p, call)) return rc;
    if (const int rc = check_grad_semiring(ctx, p, call)) return rc;
    if (const int rc = check_grad_width(ctx, p, call)) return rc;
    if (!dCval) return fail(ctx, MHS_ERR_INVALID, std::string(call) + ": null dCval");
    if (!dAval && !dBval) return fail(ctx, MHS_ERR_INVALID, std::string(call) + ": no output (dAval and dBval are both null)");
    if ((dAval && !Bval) || (dBval && !Aval))
        return fail(ctx, MHS_ERR_INVALID, std::string(call) + ": dAval needs Bval, dBval needs Aval");
    if (p->device != ctx->device) return fail(ctx, MHS_ERR_INVALID, std::string(call) + ": the plan belongs to another device");
    const ValGradArgs<V> a{{p->pat.Aptr, p->pat.Acol, Aval}, {p->pat.Bptr, p->pat.Bcol, Bval}, {p->pat.Cptr, p->pat.Ccol, dCval},
                           dAval, dBval};
    return run_values(
        ctx, p, p->gplan, ms,
        [&](hipStream_t s) {
            MHS_HIP(zero_grads(p, dAval, 0, dBval, 0, 1, s));
            return (int)MHS_OK;
        },
        [&](const ValLaunch& l, const int* list, hipStream_t s) { issue_values_grad(l, 1, a, list, s); });
}

// mhs_spgemm_values_subgrad and mhs_spgemm_values_subgrad_f32: the subgradient of a min-plus, max-plus or max-min
// plan (the rule: include/mhspgemm.h).  One pre-step -- the zero fills of ties and of the requested outputs -- then
// the backward's launch list twice: pass 1 counts the winners of every C entry into ties, pass 2 hands each winner's
// G / ties to dA and dB.  A pass's launches all precede the next pass's on the stream, so pass 2 reads final counts.
template <class V>
int spgemm_values_subgrad(mhs_ctx* ctx, mhs_values_plan* p, const V* Aval, const V* Bval, const V* Cval, const V* dCval, int* ties,
                          V* dAval, V* dBval, double* ms, const char* call) {
    if (!ctx) return MHS_ERR_INVALID;
    if (!p) return fail(ctx, MHS_ERR_INVALID, std::string(call) + ": null plan");
    if (const int rc = check_dtype<V>(ctx, p, call)) return rc;
    if (p->semiring == SR_PLUS_TIMES)
        return fail(ctx, MHS_ERR_INVALID,
                    std::string(call) + ": the plan's semiring is " + val_semiring_name(p->semiring) +
                        ", which has a gradient: mhs_spgemm_values_grad (the subgradient serves min_plus, max_plus and max_min)");
    if (const int rc = check_hard_reduce(ctx, p, call, "no subgradient")) return rc;
    if (!Aval || !Bval || !Cval || !dCval || !ties)
        return fail(ctx, MHS_ERR_INVALID,
                    std::string(call) + ": null Aval, Bval, Cval, dCval or ties (the winner test reads both operands)");
    if (!dAval && !dBval) return fail(ctx, MHS_ERR_INVALID, std::string(call) + ": no output (dAval and dBval are both null)");
    if (p->device != ctx->device) return fail(ctx, MHS_ERR_INVALID, std::string(call) + ": the plan belongs to another device");
    const ValSubArgs<V> a{{p->pat.Aptr, p->pat.Acol, Aval}, {p->pat.Bptr, p->pat.Bcol, Bval}, {p->pat.Cptr, p->pat.Ccol, Cval},
                          dCval, ties, dAval, dBval, nullptr};
    return run_values(
        ctx, p, p->gplan, ms,
        [&](hipStream_t s) {
            // ties is summed into, as dB is
            if (p->nnzC > 0) MHS_HIP(hipMemsetAsync(ties, 0, sizeof(int) * (size_t)p->nnzC, s));
            MHS_HIP(zero_grads(p, dAval, 0, dBval, 0, 1, s));
            for (int i = 0; i < p->gplan.n; ++i) {  // pass 1, whole, before run_values issues pass 2
                const ValLaunch& l = p->gplan.launch[i];
                issue_values_subgrad(l, p->semiring, 1, a, p->lists + p->list_off[l.cls], s);
            }
            return (int)MHS_OK;
        },
        [&](const ValLaunch& l, const int* list, hipStream_t s) { issue_values_subgrad(l, p->semiring, 2, a, list, s); });
}

// mhs_spgemm_values_witness and mhs_spgemm_values_witness_f32: the arg of a min-plus, max-plus or max-min plan (the
// rule: include/mhspgemm.h).  One pre-step -- wit filled with 0xFF bytes: -1 as an int, the largest unsigned -- then the
// backward's launch list once, as pass 3: every winner takes the unsigned minimum of its inner index into wit.  An
// entry no winner reaches keeps its -1: there is no post-step.
template <class V>
int spgemm_values_witness(mhs_ctx* ctx, mhs_values_plan* p, const V* Aval, const V* Bval, const V* Cval, int* wit, double* ms,
                          const char* call) {
    if (!ctx) return MHS_ERR_INVALID;
    if (!p) return fail(ctx, MHS_ERR_INVALID, std::string(call) + ": null plan");
    if (const int rc = check_dtype<V>(ctx, p, call)) return rc;
    if (p->semiring == SR_PLUS_TIMES)
        return fail(ctx, MHS_ERR_INVALID,
                    std::string(call) + ": the plan's semiring is " + val_semiring_name(p->semiring) +
                        ": a sum has no witness (the witness serves min_plus, max_plus and max_min)");
    if (const int rc = check_hard_reduce(ctx, p, call, "no witness")) return rc;
    if (!Aval || !Bval || !Cval || !wit)
        return fail(ctx, MHS_ERR_INVALID, std::string(call) + ": null Aval, Bval, Cval or wit (the winner test reads both operands)");
    if (p->device != ctx->device) return fail(ctx, MHS_ERR_INVALID, std::string(call) + ": the plan belongs to another device");
    const ValSubArgs<V> a{{p->pat.Aptr, p->pat.Acol, Aval}, {p->pat.Bptr, p->pat.Bcol, Bval}, {p->pat.Cptr, p->pat.Ccol, Cval},
                          nullptr, nullptr, nullptr, nullptr, wit};
    return run_values(
        ctx, p, p->gplan, ms,
        [&](hipStream_t s) {
            if (p->nnzC > 0) MHS_HIP(hipMemsetAsync(wit, 0xFF, sizeof(int) * (size_t)p->nnzC, s));
            return (int)MHS_OK;
        },
        [&](const ValLaunch& l, const int* list, hipStream_t s) { issue_values_subgrad(l, p->semiring, 3, a, list, s); });
}

// mhs_spgemm_values_softgrad and mhs_spgemm_values_softgrad_f32: the gradient of a smoothed plan (the rule:
// include/mhspgemm.h).  One pre-step -- the zero fills of the requested outputs -- then the backward's launch list once.
template <class V>
int spgemm_values_softgrad(mhs_ctx* ctx, mhs_values_plan* p, const V* Aval, const V* Bval, const V* Cval, const V* dCval, V* dAval,
                           V* dBval, double* ms, const char* call) {
    if (!ctx) return MHS_ERR_INVALID;
    if (!p) return fail(ctx, MHS_ERR_INVALID, std::string(call) + ": null plan");
    if (const int rc = check_dtype<V>(ctx, p, call)) return rc;
    if (p->smooth != SMOOTH_LSE)
        return fail(ctx, MHS_ERR_INVALID,
                    std::string(call) + ": the plan is not smoothed (its semiring is " + val_semiring_name(p->semiring) + "): " +
                        (p->semiring == SR_PLUS_TIMES ? "its backward is mhs_spgemm_values_grad"
                                                      : "its backward is mhs_spgemm_values_subgrad") +
                        " (the soft gradient serves plans of mhs_values_plan_create_smooth)");
    if (!Aval || !Bval || !Cval || !dCval)
        return fail(ctx, MHS_ERR_INVALID, std::string(call) + ": null Aval, Bval, Cval or dCval (every weight reads both operands)");
    if (!dAval && !dBval) return fail(ctx, MHS_ERR_INVALID, std::string(call) + ": no output (dAval and dBval are both null)");
    if (p->device != ctx->device) return fail(ctx, MHS_ERR_INVALID, std::string(call) + ": the plan belongs to another device");
    const ValSoftArgs<V> a{{p->pat.Aptr, p->pat.Acol, Aval}, {p->pat.Bptr, p->pat.Bcol, Bval}, {p->pat.Cptr, p->pat.Ccol, Cval},
                           dCval, dAval, dBval, V(0)};
    return run_values(
        ctx, p, p->gplan, ms,
        [&](hipStream_t s) {
            MHS_HIP(zero_grads(p, dAval, 0, dBval, 0, 1, s));
            return (int)MHS_OK;
        },
        [&](const ValLaunch& l, const int* list, hipStream_t s) { issue_values_softgrad(l, p->semiring, a, list, s); });
}

// mhs_spgemm_values_grad_batched / _f32: the backward of spgemm_values_batched, on a plan of any width.  Set b reads
// Aval + b * sA, Bval + b * sB and dCval + b * sG and writes dAval + b * sDA and dBval + b * sDB; the backward's
// launch list runs once per pass of up to `width` sets, as the forward's does.
template <class V>
int spgemm_values_grad_batched(mhs_ctx* ctx, mhs_values_plan* p, int nb, const V* Aval, long long sA, const V* Bval, long long sB,
                               const V* dCval, long long sG, V* dAval, long long sDA, V* dBval, long long sDB, double* ms,
                               const char* call) {
    if (!ctx) return MHS_ERR_INVALID;
    if (!p) return fail(ctx, MHS_ERR_INVALID, std::string(call) + ": null plan");
    if (const int rc = check_dtype<V>(ctx, p, call)) return rc;
    if (const int rc = check_grad_semiring(ctx, p, call)) return rc;
    if (nb < 1) return fail(ctx, MHS_ERR_INVALID, std::string(call) + ": nb = " + std::to_string(nb) + " (at least one value set)");
    if (sA < 0 || sB < 0 || sG < 0 || sDA < 0 || sDB < 0) return fail(ctx, MHS_ERR_INVALID, std::string(call) + ": negative stride");
    if ((sA > 0 && sA < p->nnzA) || (sB > 0 && sB < p->nnzB))
        return fail(ctx, MHS_ERR_INVALID,
                    std::string(call) + ": an input stride is 0 (one array shared by all sets) or at least the matrix's nnz");
    if (nb > 1 && sG < p->nnzC)
        return fail(ctx, MHS_ERR_INVALID,
                    std::string(call) + ": strideG is below nnz(C): every set has its own cotangent (a stride of 0 is not taken)");
    if (nb > 1 && ((dAval && sDA < p->nnzA) || (dBval && sDB < p->nnzB)))
        return fail(ctx, MHS_ERR_INVALID,
                    std::string(call) + ": an output stride (strideDA, strideDB) is below its matrix's nnz: gradients come back per "
                                        "set, and the sets' outputs would overlap");
    if (!dCval) return fail(ctx, MHS_ERR_INVALID, std::string(call) + ": null dCval");
    if (!dAval && !dBval) return fail(ctx, MHS_ERR_INVALID, std::string(call) + ": no output (dAval and dBval are both null)");
    if ((dAval && !Bval) || (dBval && !Aval))
        return fail(ctx, MHS_ERR_INVALID, std::string(call) + ": dAval needs Bval, dBval needs Aval");
    if (p->device != ctx->device) return fail(ctx, MHS_ERR_INVALID, std::string(call) + ": the plan belongs to another device");
    const int W = p->width, passes = (nb + W - 1) / W;
    return run_values(
        ctx, p, p->gplan, ms,
        [&](hipStream_t s) {
            MHS_HIP(zero_grads(p, dAval, sDA, dBval, sDB, nb, s));  // (over the nb segments only)
            return (int)MHS_OK;
        },
        [&](const ValLaunch& l, const int* list, hipStream_t s) {
            for (int q = 0; q < passes; ++q) {
                const long long b = (long long)q * W;
                ValGradArgs<V> a{{p->pat.Aptr, p->pat.Acol, Aval ? Aval + b * sA : nullptr},
                                 {p->pat.Bptr, p->pat.Bcol, Bval ? Bval + b * sB : nullptr},
                                 {p->pat.Cptr, p->pat.Ccol, dCval + b * sG},
                                 dAval ? dAval + b * sDA : nullptr,
                                 dBval ? dBval + b * sDB : nullptr};
                a.sA = sA, a.sB = sB, a.sG = sG, a.sDA = sDA, a.sDB = sDB;
                a.nw = nb - b < W ? (int)(nb - b) : W;
                issue_values_grad(l, W, a, list, s);
            }
        });
}

}  // namespace

int mhs_values_plan_create(mhs_ctx* ctx, const mhs_csr* A, const mhs_csr* B, const mhs_csr* C, mhs_values_plan** out) {
    return values_plan_create(ctx, A, B, C, false, MHS_MASK_PRODUCT, MHS_F64, 1, MHS_SR_PLUS_TIMES, MHS_ACC_NATIVE,
                              MHS_SMOOTH_NONE, out);
}

int mhs_values_plan_create_masked(mhs_ctx* ctx, const mhs_csr* A, const mhs_csr* B, const mhs_csr* C, int form,
                                  mhs_values_plan** out) {
    return values_plan_create(ctx, A, B, C, true, form, MHS_F64, 1, MHS_SR_PLUS_TIMES, MHS_ACC_NATIVE, MHS_SMOOTH_NONE,
                              out);
}

int mhs_values_plan_create_typed(mhs_ctx* ctx, const mhs_csr* A, const mhs_csr* B, const mhs_csr* C, int masked, int form,
                                 int dtype, mhs_values_plan** out) {
    return values_plan_create(ctx, A, B, C, masked != 0, masked ? form : (int)MHS_MASK_PRODUCT, dtype, 1, MHS_SR_PLUS_TIMES,
                              MHS_ACC_NATIVE, MHS_SMOOTH_NONE, out);
}

int mhs_values_plan_create_batched(mhs_ctx* ctx, const mhs_csr* A, const mhs_csr* B, const mhs_csr* C, int masked, int form,
                                   int dtype, int width, mhs_values_plan** out) {
    return values_plan_create(ctx, A, B, C, masked != 0, masked ? form : (int)MHS_MASK_PRODUCT, dtype, width, MHS_SR_PLUS_TIMES,
                              MHS_ACC_NATIVE, MHS_SMOOTH_NONE, out);
}

int mhs_values_plan_create_semiring(mhs_ctx* ctx, const mhs_csr* A, const mhs_csr* B, const mhs_csr* C, int masked, int form,
                                    int dtype, int semiring, mhs_values_plan** out) {
    return values_plan_create(ctx, A, B, C, masked != 0, masked ? form : (int)MHS_MASK_PRODUCT, dtype, 1, semiring, MHS_ACC_NATIVE,
                              MHS_SMOOTH_NONE, out);
}

int mhs_values_plan_create_accum(mhs_ctx* ctx, const mhs_csr* A, const mhs_csr* B, const mhs_csr* C, int masked, int form,
                                 int dtype, int width, int accum, mhs_values_plan** out) {
    return values_plan_create(ctx, A, B, C, masked != 0, masked ? form : (int)MHS_MASK_PRODUCT, dtype, width, MHS_SR_PLUS_TIMES,
                              accum, MHS_SMOOTH_NONE, out);
}

int mhs_values_plan_create_smooth(mhs_ctx* ctx, const mhs_csr* A, const mhs_csr* B, const mhs_csr* C, int masked, int form,
                                  int dtype, int semiring, int smooth, mhs_values_plan** out) {
    return values_plan_create(ctx, A, B, C, masked != 0, masked ? form : (int)MHS_MASK_PRODUCT, dtype, 1, semiring, MHS_ACC_NATIVE,
                              smooth, out);
}

int mhs_values_plan_smooth(const mhs_values_plan* p, int* smooth) {
    if (!p || !smooth) return MHS_ERR_INVALID;
    *smooth = p->smooth;
    return MHS_OK;
}

int mhs_values_plan_accum(const mhs_values_plan* p, int* accum) {
    if (!p || !accum) return MHS_ERR_INVALID;
    *accum = p->accum;
    return MHS_OK;
}

int mhs_values_plan_semiring(const mhs_values_plan* p, int* semiring) {
    if (!p || !semiring) return MHS_ERR_INVALID;
    *semiring = p->semiring;
    return MHS_OK;
}

int mhs_values_plan_width(const mhs_values_plan* p, int* width) {
    if (!p || !width) return MHS_ERR_INVALID;
    *width = p->width;
    return MHS_OK;
}

int mhs_values_plan_dtype(const mhs_values_plan* p, int* dtype) {
    if (!p || !dtype) return MHS_ERR_INVALID;
    *dtype = p->dtype;
    return MHS_OK;
}

int mhs_values_plan_kept(const mhs_values_plan* p, int64_t* kept_products) {
    if (!p || !kept_products) return MHS_ERR_INVALID;
    *kept_products = p->kept;
    return MHS_OK;
}

int mhs_spgemm_values(mhs_ctx* ctx, mhs_values_plan* p, const double* Aval, const double* Bval, double* Cval, double* ms) {
    return spgemm_values_batched<double>(ctx, p, 1, Aval, 0, Bval, 0, Cval, 0, ms, "mhs_spgemm_values");
}

int mhs_spgemm_values_f32(mhs_ctx* ctx, mhs_values_plan* p, const float* Aval, const float* Bval, float* Cval, double* ms) {
    return spgemm_values_batched<float>(ctx, p, 1, Aval, 0, Bval, 0, Cval, 0, ms, "mhs_spgemm_values_f32");
}

int mhs_spgemm_values_batched(mhs_ctx* ctx, mhs_values_plan* p, int nb, const double* Aval, int64_t strideA, const double* Bval,
                              int64_t strideB, double* Cval, int64_t strideC, double* ms) {
    return spgemm_values_batched<double>(ctx, p, nb, Aval, strideA, Bval, strideB, Cval, strideC, ms, "mhs_spgemm_values_batched");
}

int mhs_spgemm_values_batched_f32(mhs_ctx* ctx, mhs_values_plan* p, int nb, const float* Aval, int64_t strideA, const float* Bval,
                                  int64_t strideB, float* Cval, int64_t strideC, double* ms) {
    return spgemm_values_batched<float>(ctx, p, nb, Aval, strideA, Bval, strideB, Cval, strideC, ms,
                                        "mhs_spgemm_values_batched_f32");
}

int mhs_spgemm_values_grad(mhs_ctx* ctx, mhs_values_plan* p, const double* Aval, const double* Bval, const double* dCval,
                           double* dAval, double* dBval, double* ms) {
    return spgemm_values_grad<double>(ctx, p, Aval, Bval, dCval, dAval, dBval, ms, "mhs_spgemm_values_grad");
}

int mhs_spgemm_values_grad_f32(mhs_ctx* ctx, mhs_values_plan* p, const float* Aval, const float* Bval, const float* dCval,
                               float* dAval, float* dBval, double* ms) {
    return spgemm_values_grad<float>(ctx, p, Aval, Bval, dCval, dAval, dBval, ms, "mhs_spgemm_values_grad_f32");
}

int mhs_spgemm_values_grad_batched(mhs_ctx* ctx, mhs_values_plan* p, int nb, const double* Aval, int64_t strideA, const double* Bval,
                                   int64_t strideB, const double* dCval, int64_t strideG, double* dAval, int64_t strideDA,
                                   double* dBval, int64_t strideDB, double* ms) {
    return spgemm_values_grad_batched<double>(ctx, p, nb, Aval, strideA, Bval, strideB, dCval, strideG, dAval, strideDA, dBval,
                                              strideDB, ms, "mhs_spgemm_values_grad_batched");
}

int mhs_spgemm_values_grad_batched_f32(mhs_ctx* ctx, mhs_values_plan* p, int nb, const float* Aval, int64_t strideA,
                                       const float* Bval, int64_t strideB, const float* dCval, int64_t strideG, float* dAval,
                                       int64_t strideDA, float* dBval, int64_t strideDB, double* ms) {
    return spgemm_values_grad_batched<float>(ctx, p, nb, Aval, strideA, Bval, strideB, dCval, strideG, dAval, strideDA, dBval,
                                             strideDB, ms, "mhs_spgemm_values_grad_batched_f32");
}

int mhs_spgemm_values_subgrad(mhs_ctx* ctx, mhs_values_plan* p, const double* Aval, const double* Bval, const double* Cval,
                              const double* dCval, int32_t* ties, double* dAval, double* dBval, double* ms) {
    return spgemm_values_subgrad<double>(ctx, p, Aval, Bval, Cval, dCval, ties, dAval, dBval, ms, "mhs_spgemm_values_subgrad");
}

int mhs_spgemm_values_subgrad_f32(mhs_ctx* ctx, mhs_values_plan* p, const float* Aval, const float* Bval, const float* Cval,
                                  const float* dCval, int32_t* ties, float* dAval, float* dBval, double* ms) {
    return spgemm_values_subgrad<float>(ctx, p, Aval, Bval, Cval, dCval, ties, dAval, dBval, ms, "mhs_spgemm_values_subgrad_f32");
}

int mhs_spgemm_values_softgrad(mhs_ctx* ctx, mhs_values_plan* p, const double* Aval, const double* Bval, const double* Cval,
                               const double* dCval, double* dAval, double* dBval, double* ms) {
    return spgemm_values_softgrad<double>(ctx, p, Aval, Bval, Cval, dCval, dAval, dBval, ms, "mhs_spgemm_values_softgrad");
}

int mhs_spgemm_values_softgrad_f32(mhs_ctx* ctx, mhs_values_plan* p, const float* Aval, const float* Bval, const float* Cval,
                                   const float* dCval, float* dAval, float* dBval, double* ms) {
    return spgemm_values_softgrad<float>(ctx, p, Aval, Bval, Cval, dCval, dAval, dBval, ms, "mhs_spgemm_values_softgrad_f32");
}

int mhs_spgemm_values_witness(mhs_ctx* ctx, mhs_values_plan* p, const double* Aval, const double* Bval, const double* Cval,
                              int32_t* wit, double* ms) {
    return spgemm_values_witness<double>(ctx, p, Aval, Bval, Cval, wit, ms, "mhs_spgemm_values_witness");
}

int mhs_spgemm_values_witness_f32(mhs_ctx* ctx, mhs_values_plan* p, const float* Aval, const float* Bval, const float* Cval,
                                  int32_t* wit, double* ms) {
    return spgemm_values_witness<float>(ctx, p, Aval, Bval, Cval, wit, ms, "mhs_spgemm_values_witness_f32");
}

int mhs_values_plan_info(const mhs_values_plan* p, mhs_values_info* info) {
    if (!p || !info) return MHS_ERR_INVALID;
    memset(info, 0, sizeof *info);
    for (int c = 0; c < VAL_NCLASS; ++c) info->rows[c] = p->counts.rows[c];
    info->products = p->products;
    info->nnzC = p->nnzC;
    info->plan_bytes = (int64_t)(p->mem_bytes + p->tmem_bytes);
    return MHS_OK;
}

void mhs_values_plan_destroy(mhs_ctx* ctx, mhs_values_plan* p) {
    if (!p) return;
    (void)hipSetDevice(p->device);
    if (ctx && ctx->stream) (void)hipStreamSynchronize(ctx->stream);  // calls still queued read the lists
    else (void)hipDeviceSynchronize();
    for (hipEvent_t ev : p->ev)
        if (ev) (void)hipEventDestroy(ev);
    if (p->mem) (void)hipFree(p->mem);
    if (p->tmem) (void)hipFree(p->tmem);
    (void)hipGetLastError();
    delete p;
}
