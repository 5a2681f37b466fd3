// spgemm_main.cpp -- the `spgemm <file.mtx>` driver (reference src/main.cu:74-217)
// on top of the C-ABI, printing the reference's stdout lines.
//
//   spgemm [--iters K] [--warmup W] [--aat] [--vendor] [--check] [--csv DIR] [--cache] [--reuse N] [--masked N] [--grad N] [--f32] [--acc64]
//          [--batch NB] [--width W] [--semiring NAME] [--subgrad N] [--witness N] [--smooth lse] [--softgrad N] <file.mtx>
//
// Flow as in the reference: read (mmio semantics), reject non-square A unless AAT
// (exit 0, main.cu:92-96), B = A or B = A^T (AAT and not symmetric, :98-101),
// count intermediate products on the host (:102-107), H2D, run MH_spgemm, print
// per-phase times and GFLOPS = 2*flop/getTotal().  The reference's compile-time
// switches are flags here:
//   --aat     AAT=1 (inc/common.h:37): C = A * A^T (A^T built on the device)
//   --vendor  CUSPARSE=1 (inc/common.h:78): the vendor SpGEMM beside it -- rocSPARSE
//             on this box (include/mhs_vendor.h), its time and GFLOPS (:148-170)
//   --check   CHECK_RESULT=1: C == vendor C by CSR::operator== -> "pass"/"error" (:186-199)
//   --csv DIR WRITE=1: append GFLOPS to DIR/Gflops_MH-SpGEMM.csv and, with --vendor,
//             DIR/Gflops_rocsparse.csv (:173-184, :201-213; the reference's data/)
//   --cache   read <file.mtx>.mhscsr (binary CSR, stamped with the .mtx's size and
//             mtime) instead of parsing the text; written on the first run
//   --reuse N after the product, a values plan on C's pattern (mhs_values_plan_create) and N values-only
//             calls on the same A and B (mhs_spgemm_values); their mean time on a line of its own, and
//             with --check the recomputed values against the product's own by CSR::operator==
//   --masked N after the product (and --reuse), a masked values plan (mhs_values_plan_create_masked, AUTO) of
//             the same A and B on A's own pattern -- A*A kept where A has entries (an entry the file repeats is
//             one mask entry: a mask's columns ascend strictly); needs rowA = colA -- and
//             N calls; their mean time, the kept products and the dot rows on a line of its own, and with
//             --check the values against the product's own C filtered to A's pattern (the 1e-9 rule)
//   --grad N  after the product (and --reuse, --masked), a values plan on C's pattern and, with a seeded
//             cotangent G on it, N values calls and N backward calls (mhs_spgemm_values_grad, both
//             gradients); the two median times on a line of its own, and with --check the adjoint
//             identities <G, C> = <dA, Aval> = <dB, Bval> (the product is bilinear) on host-computed sums
//   --f32     a modifier of --reuse, --masked and --grad: after them, each chosen mode once more with an FP32
//             plan (mhs_values_plan_create_typed, MHS_F32) on the operands' values rounded to float, N calls
//             of mhs_spgemm_values_f32 / mhs_spgemm_values_grad_f32 beside N calls of an FP64 plan on the
//             same rounded values: one more line per mode with both times, and with --check every FP32
//             entry against the FP64 call's: within 1.01 m 2^-24 S for an entry of m kept products whose
//             absolute values sum to S (m and S from FP64 calls on all-ones and on absolute values), and
//             exactly 0 where m = 0.  Without --f32 nothing is added to the output.
//   --acc64   a modifier of --f32: after each --f32 line (--reuse, --masked, --grad, and --batch with its --grad), that
//             mode once more on a mixed plan -- float values, FP64 sums (mhs_values_plan_create_accum, MHS_F32 with
//             MHS_ACC_F64) -- with one more line ("FP32, FP64 sums") and, with --check, "values f32 acc64 pass" /
//             "... error" (likewise masked, grad, batched, grad batched).  The forward is held to the mixed plan's
//             bound against the FP64 plan on the same float-rounded values: with E the exact sum, the mixed entry is
//             within 2^-24 |E| + m 2^-53 S (1 + 2^-24) of it and the FP64 one within m 2^-53 S, so the two differ by at
//             most 1.01 (2^-24 |ref| + 2 m 2^-53 S); rows of the global class (a row of more than
//             159,744 / (8 W + 4) entries over more than 159,744 / (8 W) columns: C's float segment is their
//             accumulator) are held to the FP32 bound.  The backward is the float kernels': the FP32 bound.
//             --acc64 without --f32: the usage message.
//   --batch NB [--width W]  a modifier of --reuse: after it, NB seeded value sets of A and B on the product's
//             pattern, a plan of width W (mhs_values_plan_create_batched; 1, 2 or 4, default 4) and N calls of
//             mhs_spgemm_values_batched on all NB sets beside N x NB unbatched calls on a width-1 plan: one more
//             line with both median times (with --f32 one more, on float values), and with --check every set of
//             the batched call against the unbatched call on the same values.  FP64: both are within
//             1.01 m 2^-53 S of the exact sum, so within twice that of each other; FP32: the reference is the
//             unbatched FP64 call on the rounded values and the bound 1.01 m 2^-24 S (m from a call on all-ones;
//             the seeded values are positive, so S is the FP64 call's own result).  --batch without --reuse,
//             --width without --batch, NB < 1 or a width that is not 1, 2 or 4: the usage message.
//             With --grad N as well: after those lines, NB seeded cotangent sets beside the value sets, N calls of
//             mhs_spgemm_values_grad_batched (both gradients) on the plan of width W beside N x NB calls of
//             mhs_spgemm_values_grad on the width-1 plan: one more line per type with both median times ("values
//             grad batched"), and with --check "grad batched pass" / "grad batched error" ("grad batched f32 ..."):
//             every set of both gradients against the unbatched backward of the same type on that set -- each is
//             within 1.01 m u S of the exact sum (u = 2^-53 or 2^-24), so within twice that of the other, and
//             exactly 0 where m = 0 (m from the unbatched backward on all-ones; S: the positive values' own result).
//   --semiring NAME  a modifier of --reuse and --masked (NAME: plus_times, min_plus, max_plus or max_min): after
//             them, each chosen mode once more on a plan of that semiring (mhs_values_plan_create_semiring) on the
//             operands' values, N calls of mhs_spgemm_values, and with --f32 also on an FP32 plan on the values
//             rounded to float: one more line per mode and type with the median time, and with --check the result
//             against a sequential host loop over the products in the plan's value type, for equality (zeros equal
//             whatever their sign; plus_times, whose sums have no fixed order, to rounding of the products' absolute
//             sum): "values NAME pass" / "masked NAME pass" ("... NAME f32 pass"), or "error".
//             Without --reuse or --masked, or with another name: the usage message.  Without the switch nothing is
//             added to the output.
//   --subgrad N  a modifier of --semiring NAME (NAME not plus_times) with --reuse or --masked: after each semiring
//             values line (and its check), N subgradient calls (mhs_spgemm_values_subgrad / _f32, both gradients) on a
//             plan of that semiring, on seeded values -- quarters in [-2, 2), so that products tie -- and seeded
//             cotangents: one more line per mode and type with the median time, and with --check the call against a
//             sequential host loop of the rule (include/mhspgemm.h): the forward for equality, ties exactly, each
//             gradient entry within 1.01 (m + 1) u S of the long-double sum of its m winning weights: "values NAME
//             subgrad pass" / "masked NAME subgrad pass" ("... NAME f32 subgrad pass"), or "error".  Without --semiring,
//             with plus_times, without --reuse or --masked, or N < 1: the usage message.  Without the switch nothing
//             is added to the output.
//   --witness N  a modifier of --semiring NAME (NAME not plus_times) with --reuse or --masked, like --subgrad N and
//             after it: after each semiring values line, N witness calls (mhs_spgemm_values_witness / _f32) on a plan
//             of that semiring, on --subgrad's seeded values: one more line per mode and type with the median time,
//             and with --check the call against a sequential host loop of the rule (include/mhspgemm.h): the forward
//             for equality and per entry the smallest inner index among the products equal to it, -1 where there is
//             none: "values NAME witness pass" / "masked NAME witness pass" ("... NAME f32 witness pass"), or "error".
//             Without --semiring, with plus_times, without --reuse or --masked, or N < 1: the usage message.  Without
//             the switch nothing is added to the output.
//   --smooth lse  a modifier of --semiring min_plus | max_plus with --reuse or --masked: after the semiring lines, each
//             chosen mode once more on a smoothed plan of that semiring (mhs_values_plan_create_smooth: the reduce is
//             log-sum-exp), on seeded values uniform in [-8, 8): one more line per mode and type with the median time,
//             and with --check the result against a sequential host loop in long double at the header's bounds:
//             "values NAME lse pass" / "masked NAME lse pass" ("... NAME f32 lse pass"), or "error".  With another
//             semiring, without one, or with another word than lse: the usage message.
//   --softgrad N  a modifier of --smooth lse: after each lse line, N gradient calls (mhs_spgemm_values_softgrad / _f32,
//             both gradients) on the same plan and values, with seeded cotangents in [0.1, 1): one more line with the
//             median time, and with --check each gradient entry against the long-double sum of its exact weights on
//             the device's Cval, at the header's bound: "values NAME softgrad pass" / "masked NAME softgrad pass"
//             ("... NAME f32 softgrad pass"), or "error".  Without --smooth or N < 1: the usage message.
// Differences: W untimed warm-up calls (the reference warms the GPU with an
// empty kernel, MH_spgemm.cuh:10-25), K timed calls averaged with the context's
// workspace reused between them (the reference's iter/release loop), and an extra
// e2e line that includes Form_mask_matrix_B.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iomanip>
#include <iostream>
#include <limits>
#include <string>
#include <vector>

#include "mh_spgemm.hpp"
#include "mhs_vendor.h"

static std::string extract_matrix_name(const std::string& path) {
    const size_t s = path.find_last_of("/\\");
    std::string f = s == std::string::npos ? path : path.substr(s + 1);
    const size_t d = f.find_last_of('.');
    return d == std::string::npos ? f : f.substr(0, d);
}

static bool append_csv(const std::string& dir, const char* file, double gflops) {
    std::ofstream out(dir + "/" + file, std::ios::app);
    if (!out) {
        std::cerr << "Unable to open " << file << std::endl;
        return false;
    }
    out << std::fixed << std::setprecision(2) << gflops << std::endl;
    return true;
}

static void recycle(Tool& tools, CSR& C) {
    mhs_csr c{C.M, C.N, C.nnz, C.d_ptr, C.d_col, C.d_val};
    mhs_ctx_recycle(tools.ctx, &c);
    C.d_ptr = C.d_col = nullptr;
    C.d_val = nullptr;
}

// --masked N: A * B kept on A's pattern by a masked plan, N calls; with check against C (the full
// product, on the device) filtered to A's pattern on the host.
// A's pattern as a mask.  A mask's columns ascend strictly within a row (mhspgemm.h), and the reader keeps the
// repeated entries of a file (sorted within the row): the mask holds such a column once.  Its pattern is on the
// host (mask.ptr, mask.col); on the device it borrows A's arrays where A repeats nothing and has arrays of its
// own otherwise.  Returns whether it owns them; unborrow_mask before the mask goes out of scope.
static bool mask_of(const CSR& A, int N, CSR& mask) {
    mask.alloc(A.M, N, A.nnz);
    int n = 0;
    for (int i = 0; i < A.M; ++i) {
        mask.ptr[i] = n;
        for (int k = A.ptr[i]; k < A.ptr[i + 1]; ++k)
            if (k == A.ptr[i] || A.col[k] != A.col[k - 1]) mask.col[n++] = A.col[k];
    }
    mask.ptr[A.M] = n;
    mask.nnz = n;
    if (n == A.nnz) {
        mask.d_ptr = A.d_ptr;
        mask.d_col = A.d_col;
        return false;
    }
    mhs_shim::hip_check(hipMalloc((void**)&mask.d_ptr, sizeof(int) * (size_t)(A.M + 1)), "hipMalloc mask ptr");
    mhs_shim::hip_check(hipMalloc((void**)&mask.d_col, sizeof(int) * (size_t)(n > 0 ? n : 1)), "hipMalloc mask col");
    mhs_shim::hip_check(hipMemcpy(mask.d_ptr, mask.ptr, sizeof(int) * (size_t)(A.M + 1), hipMemcpyHostToDevice), "H2D mask ptr");
    mhs_shim::hip_check(hipMemcpy(mask.d_col, mask.col, sizeof(int) * (size_t)n, hipMemcpyHostToDevice), "H2D mask col");
    return true;
}
static void unborrow_mask(CSR& mask, bool owns) {
    if (!owns) mask.d_ptr = mask.d_col = nullptr;  // A's
}

static void run_masked(Tool& tools, const CSR& A, const CSR& B, CSR& C, int calls, bool check) {
    CSR mask;  // A's pattern with values of its own
    bool owns = false;
    try {
        owns = mask_of(A, B.N, mask);
        mhs_shim::hip_check(hipMalloc((void**)&mask.d_val, sizeof(double) * (size_t)(mask.nnz > 0 ? mask.nnz : 1)), "hipMalloc mask");
        mhs_shim::ValuesPlan plan(tools, A, B, mask, true, MHS_MASK_AUTO);
        double sum = 0;
        for (int i = 0; i < calls; ++i) {
            MH_spgemm_values(A, B, mask, plan);
            sum += plan.last_ms;
        }
        const mhs_values_info info = plan.info();
        std::printf("MH-SpGEMM masked (A's pattern) mean of %d calls is %.3lf ms, kept %lld of %lld products, dot rows %d\n", calls,
                    sum / calls, plan.kept(), (long long)info.products, (int)info.rows[7]);
        if (check) {
            C.D2H();
            std::vector<double> got((size_t)(mask.nnz > 0 ? mask.nnz : 1));
            mhs_shim::hip_check(hipMemcpy(got.data(), mask.d_val, sizeof(double) * (size_t)mask.nnz, hipMemcpyDeviceToHost), "D2H mask");
            int err = 0;
            for (int i = 0; i < mask.M; ++i)
                for (int k = mask.ptr[i]; k < mask.ptr[i + 1]; ++k) {
                    const int *row = C.col + C.ptr[i], *end = C.col + C.ptr[i + 1];
                    const int* hit = std::lower_bound(row, end, mask.col[k]);
                    const double want = hit != end && *hit == mask.col[k] ? C.val[hit - C.col] : 0.0;
                    const double d = std::fabs(want - got[(size_t)k]);
                    if (!(d < 1e-9 || d < 1e-9 * std::fabs(want))) ++err;
                }
            std::puts(err == 0 ? "masked pass" : "masked fail");
        }
    } catch (const std::exception&) {
        std::puts("masked fail");
    }
    unborrow_mask(mask, owns);  // (the mask's own arrays go with it)
}

static double median(std::vector<double> v) {
    std::sort(v.begin(), v.end());
    return v.empty() ? 0.0 : 0.5 * (v[(v.size() - 1) / 2] + v[v.size() / 2]);
}

// --grad N: the backward of the values call on C's own pattern, N calls beside N values calls; with check the
// adjoint identities.  Both sides of an identity are the same terms a * b * g summed in another order, so they
// agree to rounding: the bound is 1e-9 of the sums of the absolute per-entry terms.
static void run_grad(Tool& tools, const CSR& A, const CSR& B, CSR& C, int calls, bool check) {
    double *dG = nullptr, *dA = nullptr, *dB = nullptr;
    const size_t nA = (size_t)A.nnz, nB = (size_t)B.nnz, nC = (size_t)C.nnz;
    try {
        std::vector<double> G(nC ? nC : 1);
        unsigned long long state = 0x9e3779b97f4a7c15ULL;  // the seed
        for (size_t s = 0; s < nC; ++s) {
            state = state * 6364136223846793005ULL + 1442695040888963407ULL;
            G[s] = 0.1 + 0.9 * (double)(state >> 11) / 9007199254740992.0;
        }
        mhs_shim::hip_check(hipMalloc((void**)&dG, sizeof(double) * (nC ? nC : 1)), "hipMalloc G");
        mhs_shim::hip_check(hipMalloc((void**)&dA, sizeof(double) * (nA ? nA : 1)), "hipMalloc dA");
        mhs_shim::hip_check(hipMalloc((void**)&dB, sizeof(double) * (nB ? nB : 1)), "hipMalloc dB");
        mhs_shim::hip_check(hipMemcpy(dG, G.data(), sizeof(double) * nC, hipMemcpyHostToDevice), "H2D G");
        mhs_shim::ValuesPlan plan(tools, A, B, C);
        std::vector<double> fwd, bwd;
        for (int i = 0; i < calls; ++i) {
            MH_spgemm_values(A, B, C, plan);
            fwd.push_back(plan.last_ms);
        }
        for (int i = 0; i < calls; ++i) {
            MH_spgemm_values_grad(A, B, dG, dA, dB, plan);
            bwd.push_back(plan.last_ms);
        }
        std::printf("MH-SpGEMM values backward (both gradients) median of %d calls is %.3lf ms, the values call's %.3lf ms\n", calls,
                    median(bwd), median(fwd));
        if (check) {
            C.D2H();
            std::vector<double> gA(nA ? nA : 1), gB(nB ? nB : 1);
            mhs_shim::hip_check(hipMemcpy(gA.data(), dA, sizeof(double) * nA, hipMemcpyDeviceToHost), "D2H dA");
            mhs_shim::hip_check(hipMemcpy(gB.data(), dB, sizeof(double) * nB, hipMemcpyDeviceToHost), "D2H dB");
            long double gc = 0, ga = 0, gb = 0, ac = 0, aa = 0, ab = 0;
            for (size_t s = 0; s < nC; ++s) gc += (long double)G[s] * C.val[s], ac += std::fabs(G[s] * C.val[s]);
            for (size_t p = 0; p < nA; ++p) ga += (long double)gA[p] * A.val[p], aa += std::fabs(gA[p] * A.val[p]);
            for (size_t q = 0; q < nB; ++q) gb += (long double)gB[q] * B.val[q], ab += std::fabs(gB[q] * B.val[q]);
            const bool ok = std::fabs((double)(gc - ga)) <= 1e-9 * (double)(ac + aa) && std::fabs((double)(gc - gb)) <= 1e-9 * (double)(ac + ab);
            std::printf("<G,C> = %.12e, <dA,A> = %.12e, <dB,B> = %.12e\n", (double)gc, (double)ga, (double)gb);
            std::puts(ok ? "grad pass" : "grad error");
        }
    } catch (const std::exception&) {
        std::puts("grad error");
    }
    (void)hipFree(dG);
    (void)hipFree(dA);
    (void)hipFree(dB);
}

// ---- --f32: the values modes once more on float values, beside an FP64 plan on the same rounded values
template <class T>
struct DevArr {  // a device array of n entries (at least one allocated)
    T* p = nullptr;
    size_t n;
    explicit DevArr(size_t n_) : n(n_) { mhs_shim::hip_check(hipMalloc((void**)&p, sizeof(T) * (n ? n : 1)), "hipMalloc (--f32)"); }
    DevArr(const DevArr&) = delete;
    DevArr& operator=(const DevArr&) = delete;
    ~DevArr() { (void)hipFree(p); }
    void put(const std::vector<T>& v) { mhs_shim::hip_check(hipMemcpy(p, v.data(), sizeof(T) * n, hipMemcpyHostToDevice), "H2D (--f32)"); }
    std::vector<T> get() const {
        std::vector<T> v(n ? n : 1);
        mhs_shim::hip_check(hipMemcpy(v.data(), p, sizeof(T) * n, hipMemcpyDeviceToHost), "D2H (--f32)");
        v.resize(n);
        return v;
    }
};

static void f32_ok(mhs_ctx* ctx, int rc) {
    if (rc != MHS_OK) throw std::runtime_error(mhs_last_error(ctx));
}

// |got - ref| <= 1.01 m 2^-24 S per entry, exactly 0 where m = 0, no NaN (m, S: the FP64 call on ones / on absolute values)
static bool f32_within(const std::vector<float>& got, const std::vector<double>& ref, const std::vector<double>& m,
                       const std::vector<double>& S) {
    for (size_t i = 0; i < got.size(); ++i) {
        const double mm = std::floor(m[i] + 0.5), d = std::fabs((double)got[i] - ref[i]);
        if (mm == 0 ? got[i] != 0.0f : !(d <= 1.01 * mm * 5.9604644775390625e-8 * S[i])) return false;
    }
    return true;
}

// The forward of a mixed plan (FP32 values, FP64 sums) of width `width` against the FP64 call on the same values:
// |got - ref| <= 1.01 (2^-24 |ref| + 2 m 2^-53 S) per entry, exactly 0 where m = 0; the rows the plan sends to its
// global class -- by the plan's rule at 8 x width sum bytes, restated here on P's host pattern -- within the FP32 bound.
// The restated rule is held against the plan: its rows must number plan_global, mhs_values_info's rows[6] (a masked
// plan's dot rows come before the rule, so there the plan may count fewer); otherwise the check fails.
static bool acc64_global_row(const CSR& P, int i, int width) {
    const int s = P.ptr[i], n = P.ptr[i + 1] - s, sb = 8 * width, block_bytes = 159744;
    if (n <= 0) return false;
    const long long span = (long long)P.col[s + n - 1] - P.col[s] + 1;
    return span > block_bytes / sb && n > (block_bytes / (sb + 4) & ~1);
}
static bool acc64_within(const CSR& P, int width, int plan_global, bool masked, const float* got, const std::vector<double>& ref,
                         const std::vector<double>& m, const std::vector<double>& S) {
    int restated = 0;
    for (int i = 0; i < P.M; ++i) restated += acc64_global_row(P, i, width);
    if (masked ? restated < plan_global : restated != plan_global) return false;
    for (int i = 0; i < P.M; ++i) {
        const bool global = acc64_global_row(P, i, width);
        for (int q = P.ptr[i]; q < P.ptr[i + 1]; ++q) {
            const double mm = std::floor(m[q] + 0.5), d = std::fabs((double)got[q] - ref[q]);
            const double bound = global ? 1.01 * mm * 5.9604644775390625e-8 * S[q]
                                        : 1.01 * (5.9604644775390625e-8 * std::fabs(ref[q]) + 2 * mm * 1.1102230246251565e-16 * S[q]);
            if (mm == 0 ? got[q] != 0.0f : !(d <= bound)) return false;
        }
    }
    return true;
}

// One mode: plans of both types for A * B on P's pattern (masked: a mask), `calls` calls of each -- the values
// call, or (backward) the backward call with both gradients on a seeded cotangent -- and the check.
// acc64: the FP32 plan is a mixed one (FP64 sums); P's host pattern is then read by the forward's check.
static void run_f32(Tool& tools, const CSR& A, const CSR& B, const CSR& P, bool masked, bool backward, int calls, bool check,
                    const char* label, const char* tag, bool acc64 = false) {
    const char* sfx = acc64 ? " acc64" : "";
    try {
        const size_t nA = (size_t)A.nnz, nB = (size_t)B.nnz, nC = (size_t)P.nnz;
        auto rounded = [](const double* v, size_t n) {
            std::vector<float> f(n);
            for (size_t i = 0; i < n; ++i) f[i] = (float)v[i];
            return f;
        };
        std::vector<double> G(nC);
        unsigned long long state = 0x9e3779b97f4a7c15ULL;  // the seed
        for (size_t s = 0; s < nC; ++s) {
            state = state * 6364136223846793005ULL + 1442695040888963407ULL;
            G[s] = 0.1 + 0.9 * (double)(state >> 11) / 9007199254740992.0;
        }
        const std::vector<float> a32 = rounded(A.val, nA), b32 = rounded(B.val, nB), g32 = rounded(G.data(), nC);
        mhs_shim::ValuesPlan p32(tools, A, B, P, masked, MHS_MASK_AUTO, MHS_F32, 1, MHS_SR_PLUS_TIMES, acc64 ? MHS_ACC_F64 : MHS_ACC_NATIVE);
        mhs_shim::ValuesPlan p64(tools, A, B, P, masked, MHS_MASK_AUTO, MHS_F64);
        DevArr<float> fa(nA), fb(nB), fg(nC), fc(nC), fda(nA), fdb(nB);
        DevArr<double> da(nA), db(nB), dg(nC), dc(nC), dda(nA), ddb(nB);
        fa.put(a32), fb.put(b32), fg.put(g32);
        // the FP64 call on values made of the rounded ones by f: what it returns, per output
        struct Out {
            std::vector<double> c, a, b;
        };
        auto call64 = [&](double (*f)(float), double* ms) {
            std::vector<double> va(nA), vb(nB), vg(nC);
            for (size_t i = 0; i < nA; ++i) va[i] = f(a32[i]);
            for (size_t i = 0; i < nB; ++i) vb[i] = f(b32[i]);
            for (size_t i = 0; i < nC; ++i) vg[i] = f(g32[i]);
            da.put(va), db.put(vb), dg.put(vg);
            if (backward) f32_ok(p64.ctx, mhs_spgemm_values_grad(p64.ctx, p64.plan, da.p, db.p, dg.p, dda.p, ddb.p, ms));
            else f32_ok(p64.ctx, mhs_spgemm_values(p64.ctx, p64.plan, da.p, db.p, dc.p, ms));
            return backward ? Out{{}, dda.get(), ddb.get()} : Out{dc.get(), {}, {}};
        };
        std::vector<double> t32, t64;
        Out ref;
        for (int i = 0; i < calls; ++i) {
            if (backward) MH_spgemm_values_grad(fa.p, fb.p, fg.p, fda.p, fdb.p, p32);
            else MH_spgemm_values(fa.p, fb.p, fc.p, p32);
            t32.push_back(p32.last_ms);
        }
        for (int i = 0; i < calls; ++i) {
            double ms = 0;
            ref = call64([](float x) { return (double)x; }, &ms);
            t64.push_back(ms);
        }
        std::printf("MH-SpGEMM %s FP32%s median of %d calls is %.3lf ms, FP64 on the same rounded values %.3lf ms\n", label,
                    acc64 ? ", FP64 sums" : "", calls, median(t32), median(t64));
        if (check) {
            const Out m = call64([](float) { return 1.0; }, nullptr), S = call64([](float x) { return std::fabs((double)x); }, nullptr);
            const bool ok = backward ? f32_within(fda.get(), ref.a, m.a, S.a) && f32_within(fdb.get(), ref.b, m.b, S.b)
                            : acc64  ? acc64_within(P, 1, p32.info().rows[6], masked, fc.get().data(), ref.c, m.c, S.c)
                                     : f32_within(fc.get(), ref.c, m.c, S.c);
            std::printf("%s f32%s %s\n", tag, sfx, ok ? "pass" : "error");
        }
    } catch (const std::exception&) {
        std::printf("%s f32%s error\n", tag, sfx);
    }
}

// ---- --semiring NAME: a values mode once more on a plan of that semiring, in T (double, or float on rounded values)
static const char* const SEMIRING_NAMES[4] = {"plus_times", "min_plus", "max_plus", "max_min"};
static int semiring_of(const char* name) {
    for (int s = 0; s < 4; ++s)
        if (!std::strcmp(name, SEMIRING_NAMES[s])) return s;
    return -1;
}
static int semiring_call(mhs_shim::ValuesPlan& p, const double* a, const double* b, double* c) {
    return mhs_spgemm_values(p.ctx, p.plan, a, b, c, &p.last_ms);
}
static int semiring_call(mhs_shim::ValuesPlan& p, const float* a, const float* b, float* c) {
    return mhs_spgemm_values_f32(p.ctx, p.plan, a, b, c, &p.last_ms);
}
// The sequential reference: every product of A's and B's entries in their order, reduced into its slot of P's row.
// mag (plus_times): per entry the sum of its products' absolute values, what a sum's rounding is measured against
template <class T>
static std::vector<T> semiring_host(int sr, const CSR& A, const CSR& B, const CSR& P, const std::vector<T>& av,
                                    const std::vector<T>& bv, std::vector<double>& mag) {
    const T inf = std::numeric_limits<T>::infinity();
    const T identity = sr == MHS_SR_PLUS_TIMES ? T(0) : sr == MHS_SR_MIN_PLUS ? inf : -inf;
    std::vector<T> c((size_t)P.nnz, identity);
    mag.assign((size_t)P.nnz, 0.0);
    for (int i = 0; i < A.M; ++i) {
        const int *row = P.col + P.ptr[i], *end = P.col + P.ptr[i + 1];
        for (int k = A.ptr[i]; k < A.ptr[i + 1]; ++k)
            for (int j = B.ptr[A.col[k]]; j < B.ptr[A.col[k] + 1]; ++j) {
                const int* hit = std::lower_bound(row, end, B.col[j]);
                if (hit == end || *hit != B.col[j]) continue;  // (outside a mask)
                T& x = c[(size_t)(hit - P.col)];
                const T a = av[(size_t)k], b = bv[(size_t)j];
                if (sr == MHS_SR_PLUS_TIMES) x += a * b, mag[(size_t)(hit - P.col)] += std::fabs((double)a * (double)b);
                else if (sr == MHS_SR_MIN_PLUS) x = std::min(x, a + b);
                else if (sr == MHS_SR_MAX_PLUS) x = std::max(x, a + b);
                else x = std::max(x, std::min(a, b));
            }
    }
    return c;
}
// P: the plan's C pattern, with its host arrays (masked: a mask)
template <class T>
static void run_semiring(Tool& tools, const CSR& A, const CSR& B, const CSR& P, bool masked, int sr, int calls, bool check,
                         const char* label, const char* tag) {
    const bool f32 = sizeof(T) == sizeof(float);
    const char* name = SEMIRING_NAMES[sr];
    try {
        const size_t nA = (size_t)A.nnz, nB = (size_t)B.nnz, nC = (size_t)P.nnz;
        std::vector<T> av(nA), bv(nB);
        for (size_t i = 0; i < nA; ++i) av[i] = (T)A.val[i];
        for (size_t i = 0; i < nB; ++i) bv[i] = (T)B.val[i];
        mhs_shim::ValuesPlan plan(tools, A, B, P, masked, MHS_MASK_AUTO, f32 ? MHS_F32 : MHS_F64, 1, sr);
        DevArr<T> da(nA), db(nB), dc(nC);
        da.put(av), db.put(bv);
        std::vector<double> t;
        for (int i = 0; i < calls; ++i) {
            f32_ok(plan.ctx, semiring_call(plan, da.p, db.p, dc.p));
            t.push_back(plan.last_ms);
        }
        std::printf("MH-SpGEMM %s %s %s median of %d calls is %.3lf ms\n", label, name, f32 ? "FP32" : "FP64", calls, median(t));
        if (check) {
            // (plus_times sums in another order than the kernels, so to rounding: equality is the other three's contract)
            std::vector<double> mag;
            const std::vector<T> want = semiring_host<T>(sr, A, B, P, av, bv, mag), got = dc.get();
            bool ok = got.size() == want.size();
            for (size_t i = 0; ok && i < nC; ++i) {
                const double g = (double)got[i], w = (double)want[i];
                ok = sr == MHS_SR_PLUS_TIMES ? std::fabs(g - w) <= (f32 ? 1e-4 : 1e-12) * mag[i] : got[i] == want[i];
            }
            std::printf("%s %s%s %s\n", tag, name, f32 ? " f32" : "", ok ? "pass" : "error");
        }
    } catch (const std::exception&) {
        std::printf("%s %s%s error\n", tag, name, f32 ? " f32" : "");
    }
}

// ---- --subgrad N: the subgradient of a semiring values mode (mhs_spgemm_values_subgrad / _f32), in T
static int subgrad_call(mhs_shim::ValuesPlan& p, const double* a, const double* b, const double* c, const double* g, int32_t* t,
                        double* da, double* db) {
    return mhs_spgemm_values_subgrad(p.ctx, p.plan, a, b, c, g, t, da, db, &p.last_ms);
}
static int subgrad_call(mhs_shim::ValuesPlan& p, const float* a, const float* b, const float* c, const float* g, int32_t* t,
                        float* da, float* db) {
    return mhs_spgemm_values_subgrad_f32(p.ctx, p.plan, a, b, c, g, t, da, db, &p.last_ms);
}
// One plan of semiring sr (not plus_times) for A * B on P's pattern (masked: a mask): seeded values -- quarters in
// [-2, 2), so that products tie -- and seeded cotangents in [0.1, 1), one values call for Cval and `calls` subgradient
// calls (both gradients).  check: a sequential host loop of the rule over the products in T -- the forward for
// equality, ties exactly, and each gradient entry within 1.01 (m + 1) u S of the long-double sum of its m winning
// weights, S the sum of their absolute values; exactly 0 where m = 0.
template <class T>
static void run_subgrad(Tool& tools, const CSR& A, const CSR& B, const CSR& P, bool masked, int sr, int calls, bool check,
                        const char* label, const char* tag) {
    const bool f32 = sizeof(T) == sizeof(float);
    const char* name = SEMIRING_NAMES[sr];
    try {
        const size_t nA = (size_t)A.nnz, nB = (size_t)B.nnz, nC = (size_t)P.nnz;
        unsigned long long state = 0x9e3779b97f4a7c15ULL;  // the seed
        auto next = [&]() {
            state = state * 6364136223846793005ULL + 1442695040888963407ULL;
            return state >> 11;
        };
        std::vector<T> av(nA), bv(nB), gv(nC);
        for (T& x : av) x = (T)(((int)(next() % 16) - 8) * 0.25);
        for (T& x : bv) x = (T)(((int)(next() % 16) - 8) * 0.25);
        for (T& x : gv) x = (T)(0.1 + 0.9 * (double)next() / 9007199254740992.0);
        mhs_shim::ValuesPlan plan(tools, A, B, P, masked, MHS_MASK_AUTO, f32 ? MHS_F32 : MHS_F64, 1, sr);
        DevArr<T> da(nA), db(nB), dc(nC), dg(nC), dda(nA), ddb(nB);
        DevArr<int32_t> dt(nC);
        da.put(av), db.put(bv), dg.put(gv);
        f32_ok(plan.ctx, semiring_call(plan, da.p, db.p, dc.p));
        std::vector<double> t;
        for (int i = 0; i < calls; ++i) {
            f32_ok(plan.ctx, subgrad_call(plan, da.p, db.p, dc.p, dg.p, dt.p, dda.p, ddb.p));
            t.push_back(plan.last_ms);
        }
        std::printf("MH-SpGEMM %s %s subgradient %s (both gradients) median of %d calls is %.3lf ms\n", label, name,
                    f32 ? "FP32" : "FP64", calls, median(t));
        if (check) {
            std::vector<double> mag;
            const std::vector<T> c = semiring_host<T>(sr, A, B, P, av, bv, mag), gotC = dc.get(), gotA = dda.get(), gotB = ddb.get();
            const std::vector<int32_t> gotT = dt.get();
            const T inf = std::numeric_limits<T>::infinity(), identity = sr == MHS_SR_MIN_PLUS ? inf : -inf;
            // every kept product in the host's order: fn(A entry, B entry, C position, whether it wins)
            auto walk = [&](auto fn) {
                for (int i = 0; i < A.M; ++i) {
                    const int *row = P.col + P.ptr[i], *end = P.col + P.ptr[i + 1];
                    for (int k = A.ptr[i]; k < A.ptr[i + 1]; ++k)
                        for (int j = B.ptr[A.col[k]]; j < B.ptr[A.col[k] + 1]; ++j) {
                            const int* hit = std::lower_bound(row, end, B.col[j]);
                            if (hit == end || *hit != B.col[j]) continue;  // (outside a mask)
                            const size_t s = (size_t)(hit - P.col);
                            const T a = av[(size_t)k], b = bv[(size_t)j], prod = sr == MHS_SR_MAX_MIN ? std::min(a, b) : a + b;
                            fn((size_t)k, (size_t)j, s, prod == c[s] && c[s] != identity);
                        }
                }
            };
            std::vector<int32_t> ties(nC, 0);
            walk([&](size_t, size_t, size_t s, bool win) { ties[s] += win ? 1 : 0; });
            struct Sum {
                long double x = 0, S = 0;
                int m = 0;
            };
            std::vector<Sum> wa(nA), wb(nB);
            auto add = [](Sum& e, long double w) { e.x += w, e.S += std::fabs(w), ++e.m; };
            walk([&](size_t k, size_t j, size_t s, bool win) {
                if (!win) return;
                const long double w = (long double)gv[s] / (long double)ties[s];
                const T a = av[k], b = bv[j];
                if (sr != MHS_SR_MAX_MIN) add(wa[k], w), add(wb[j], w);
                else if (a < b) add(wa[k], w);
                else if (b < a) add(wb[j], w);
                else add(wa[k], w / 2), add(wb[j], w / 2);
            });
            const long double u = f32 ? 5.9604644775390625e-8L : 1.1102230246251565e-16L;
            auto within = [&](const std::vector<T>& got, const std::vector<Sum>& want) {
                for (size_t i = 0; i < want.size(); ++i) {
                    const long double d = std::fabs((long double)got[i] - want[i].x);
                    if (want[i].m == 0 ? got[i] != T(0) : !(d <= 1.01L * (want[i].m + 1) * u * want[i].S)) return false;
                }
                return true;
            };
            bool ok = gotC.size() == c.size() && gotT == ties;
            for (size_t i = 0; ok && i < nC; ++i) ok = gotC[i] == c[i];
            ok = ok && within(gotA, wa) && within(gotB, wb);
            std::printf("%s %s%s subgrad %s\n", tag, name, f32 ? " f32" : "", ok ? "pass" : "error");
        }
    } catch (const std::exception&) {
        std::printf("%s %s%s subgrad error\n", tag, name, f32 ? " f32" : "");
    }
}

// ---- --witness N: the arg of a semiring values mode (mhs_spgemm_values_witness / _f32), in T
static int witness_call(mhs_shim::ValuesPlan& p, const double* a, const double* b, const double* c, int32_t* w) {
    return mhs_spgemm_values_witness(p.ctx, p.plan, a, b, c, w, &p.last_ms);
}
static int witness_call(mhs_shim::ValuesPlan& p, const float* a, const float* b, const float* c, int32_t* w) {
    return mhs_spgemm_values_witness_f32(p.ctx, p.plan, a, b, c, w, &p.last_ms);
}
// One plan of semiring sr (not plus_times) for A * B on P's pattern (masked: a mask): run_subgrad's seeded values --
// quarters in [-2, 2), so that products tie -- one values call for Cval and `calls` witness calls.  check: a sequential
// host loop of the rule over the products in T -- the forward for equality, and per entry the smallest inner index
// among the products equal to it (-1: none, or the entry is the identity), for equality.
template <class T>
static void run_witness(Tool& tools, const CSR& A, const CSR& B, const CSR& P, bool masked, int sr, int calls, bool check,
                        const char* label, const char* tag) {
    const bool f32 = sizeof(T) == sizeof(float);
    const char* name = SEMIRING_NAMES[sr];
    try {
        const size_t nA = (size_t)A.nnz, nB = (size_t)B.nnz, nC = (size_t)P.nnz;
        unsigned long long state = 0x9e3779b97f4a7c15ULL;  // the seed
        auto next = [&]() {
            state = state * 6364136223846793005ULL + 1442695040888963407ULL;
            return state >> 11;
        };
        std::vector<T> av(nA), bv(nB);
        for (T& x : av) x = (T)(((int)(next() % 16) - 8) * 0.25);
        for (T& x : bv) x = (T)(((int)(next() % 16) - 8) * 0.25);
        mhs_shim::ValuesPlan plan(tools, A, B, P, masked, MHS_MASK_AUTO, f32 ? MHS_F32 : MHS_F64, 1, sr);
        DevArr<T> da(nA), db(nB), dc(nC);
        DevArr<int32_t> dw(nC);
        da.put(av), db.put(bv);
        f32_ok(plan.ctx, semiring_call(plan, da.p, db.p, dc.p));
        std::vector<double> t;
        for (int i = 0; i < calls; ++i) {
            f32_ok(plan.ctx, witness_call(plan, da.p, db.p, dc.p, dw.p));
            t.push_back(plan.last_ms);
        }
        std::printf("MH-SpGEMM %s %s witness %s median of %d calls is %.3lf ms\n", label, name, f32 ? "FP32" : "FP64", calls,
                    median(t));
        if (check) {
            std::vector<double> mag;
            const std::vector<T> c = semiring_host<T>(sr, A, B, P, av, bv, mag), gotC = dc.get();
            const std::vector<int32_t> gotW = dw.get();
            const T inf = std::numeric_limits<T>::infinity(), identity = sr == MHS_SR_MIN_PLUS ? inf : -inf;
            std::vector<int32_t> wit(nC, -1);
            for (int i = 0; i < A.M; ++i) {
                const int *row = P.col + P.ptr[i], *end = P.col + P.ptr[i + 1];
                for (int k = A.ptr[i]; k < A.ptr[i + 1]; ++k)
                    for (int j = B.ptr[A.col[k]]; j < B.ptr[A.col[k] + 1]; ++j) {
                        const int* hit = std::lower_bound(row, end, B.col[j]);
                        if (hit == end || *hit != B.col[j]) continue;  // (outside a mask)
                        const size_t s = (size_t)(hit - P.col);
                        const T a = av[(size_t)k], b = bv[(size_t)j], prod = sr == MHS_SR_MAX_MIN ? std::min(a, b) : a + b;
                        if (prod == c[s] && c[s] != identity && (wit[s] < 0 || A.col[k] < wit[s])) wit[s] = A.col[k];
                    }
            }
            bool ok = gotC.size() == c.size() && gotW == wit;
            for (size_t i = 0; ok && i < nC; ++i) ok = gotC[i] == c[i];
            std::printf("%s %s%s witness %s\n", tag, name, f32 ? " f32" : "", ok ? "pass" : "error");
        }
    } catch (const std::exception&) {
        std::printf("%s %s%s witness error\n", tag, name, f32 ? " f32" : "");
    }
}

// ---- --smooth lse [--softgrad N]: a min-plus or max-plus values mode once more on a smoothed plan
// (mhs_values_plan_create_smooth), and its gradient (mhs_spgemm_values_softgrad / _f32), in T
static int softgrad_call(mhs_shim::ValuesPlan& p, const double* a, const double* b, const double* c, const double* g, double* da,
                         double* db) {
    return mhs_spgemm_values_softgrad(p.ctx, p.plan, a, b, c, g, da, db, &p.last_ms);
}
static int softgrad_call(mhs_shim::ValuesPlan& p, const float* a, const float* b, const float* c, const float* g, float* da,
                         float* db) {
    return mhs_spgemm_values_softgrad_f32(p.ctx, p.plan, a, b, c, g, da, db, &p.last_ms);
}
// One smoothed plan of semiring sr (min_plus or max_plus) for A * B on P's pattern (masked: a mask): seeded values
// uniform in [-8, 8) and seeded cotangents in [0.1, 1); `calls` values calls, then `grads` softgrad calls (both
// gradients; 0: none).  check: a sequential host loop in long double over the products v = a + b formed in T, at the
// header's bounds (include/mhspgemm.h, "soft semiring plans") -- the forward at the bound of the team, wave, block and
// dot rows, and at the larger of that and the global rows' bound where the plan has rows of the global class (the CLI
// does not know which rows they are); the gradient, on the Cval the device computed, at the softgrad bound.
template <class T>
static void run_soft(Tool& tools, const CSR& A, const CSR& B, const CSR& P, bool masked, int sr, int calls, int grads, bool check,
                     const char* label, const char* tag) {
    const bool f32 = sizeof(T) == sizeof(float);
    const char* name = SEMIRING_NAMES[sr];
    const char* stage = "lse";
    try {
        const size_t nA = (size_t)A.nnz, nB = (size_t)B.nnz, nC = (size_t)P.nnz;
        unsigned long long state = 0x9e3779b97f4a7c15ULL;  // the seed
        auto next = [&]() {
            state = state * 6364136223846793005ULL + 1442695040888963407ULL;
            return state >> 11;
        };
        auto unit = [&]() { return (double)next() / 9007199254740992.0; };
        std::vector<T> av(nA), bv(nB), gv(nC);
        for (T& x : av) x = (T)(16.0 * unit() - 8.0);
        for (T& x : bv) x = (T)(16.0 * unit() - 8.0);
        for (T& x : gv) x = (T)(0.1 + 0.9 * unit());
        mhs_shim::ValuesPlan plan(tools, A, B, P, masked, MHS_MASK_AUTO, f32 ? MHS_F32 : MHS_F64, 1, sr, MHS_ACC_NATIVE, MHS_SMOOTH_LSE);
        DevArr<T> da(nA), db(nB), dc(nC), dg(nC), dda(nA), ddb(nB);
        da.put(av), db.put(bv), dg.put(gv);
        std::vector<double> t;
        for (int i = 0; i < calls; ++i) {
            f32_ok(plan.ctx, semiring_call(plan, da.p, db.p, dc.p));
            t.push_back(plan.last_ms);
        }
        std::printf("MH-SpGEMM %s %s lse %s median of %d calls is %.3lf ms\n", label, name, f32 ? "FP32" : "FP64", calls, median(t));
        const long double u = f32 ? 5.9604644775390625e-8L : 1.1102230246251565e-16L, sg = sr == MHS_SR_MIN_PLUS ? -1.0L : 1.0L;
        const long double c_exp = 2, c_log = f32 ? 4 : 2;  // (the device library's, measured: include/mhspgemm.h)
        // every kept product in the host's order: fn(A entry, B entry, C position, the signed product formed in T)
        auto walk = [&](auto fn) {
            for (int i = 0; i < A.M; ++i) {
                const int *row = P.col + P.ptr[i], *end = P.col + P.ptr[i + 1];
                for (int k = A.ptr[i]; k < A.ptr[i + 1]; ++k)
                    for (int j = B.ptr[A.col[k]]; j < B.ptr[A.col[k] + 1]; ++j) {
                        const int* hit = std::lower_bound(row, end, B.col[j]);
                        if (hit == end || *hit != B.col[j]) continue;  // (outside a mask)
                        const T v = av[(size_t)k] + bv[(size_t)j];
                        fn((size_t)k, (size_t)j, (size_t)(hit - P.col), sg * (long double)v);
                    }
            }
        };
        const std::vector<T> gotC = dc.get();
        if (check) {
            const long double ninf = -std::numeric_limits<long double>::infinity();
            std::vector<long double> M(nC, ninf), sum(nC, 0.0L), V(nC, 0.0L);
            std::vector<int> m(nC, 0);
            walk([&](size_t, size_t, size_t s, long double v) { M[s] = std::max(M[s], v), V[s] = std::max(V[s], std::fabs(v)), ++m[s]; });
            walk([&](size_t, size_t, size_t s, long double v) { sum[s] += std::exp(v - M[s]); });
            const bool has_global = plan.info().rows[6] > 0;
            bool ok = gotC.size() == nC;
            for (size_t s = 0; ok && s < nC; ++s) {
                if (m[s] == 0) {
                    ok = (long double)gotC[s] == sg * ninf;  // the identity
                    continue;
                }
                const long double E = sg * (M[s] + std::log(sum[s])), lnm = std::log((long double)m[s]);
                long double bound = 1.01L * u * (std::fabs(E) + 2 * m[s] + 2 * c_exp + 2 * c_log * lnm);
                if (has_global) bound = std::max(bound, 1.01L * m[s] * u * (V[s] + lnm + 2 * c_exp + 2 * c_log + 1));
                ok = std::fabs((long double)gotC[s] - E) <= bound;
            }
            std::printf("%s %s%s lse %s\n", tag, name, f32 ? " f32" : "", ok ? "pass" : "error");
        }
        if (grads <= 0) return;
        stage = "softgrad";
        t.clear();
        for (int i = 0; i < grads; ++i) {
            f32_ok(plan.ctx, softgrad_call(plan, da.p, db.p, dc.p, dg.p, dda.p, ddb.p));
            t.push_back(plan.last_ms);
        }
        std::printf("MH-SpGEMM %s %s lse gradient %s (both gradients) median of %d calls is %.3lf ms\n", label, name,
                    f32 ? "FP32" : "FP64", grads, median(t));
        if (check) {
            struct Sum {
                long double x = 0, S = 0, D = 0;
                int m = 0;
            };
            std::vector<Sum> wa(nA), wb(nB);
            auto add = [](Sum& e, long double w, long double d) { e.x += w, e.S += std::fabs(w), e.D = std::max(e.D, std::fabs(d)), ++e.m; };
            walk([&](size_t k, size_t j, size_t s, long double v) {
                const long double c = sg * (long double)gotC[s];
                if (!std::isfinite(c)) return add(wa[k], 0, 0), add(wb[j], 0, 0);
                const long double w = (long double)gv[s] * std::exp(v - c);
                add(wa[k], w, v - c), add(wb[j], w, v - c);
            });
            const long double flush = f32 ? 1.1754943508222875e-38L : 0.0L;  // 2^-126 x max |G| (< 1): a subnormal weight may flush
            auto within = [&](const std::vector<T>& got, const std::vector<Sum>& want) {
                for (size_t i = 0; i < want.size(); ++i) {
                    const long double d = std::fabs((long double)got[i] - want[i].x);
                    const long double bound = 1.01L * (want[i].m + want[i].D + 2 * c_exp + 1) * u * want[i].S + want[i].m * flush;
                    if (want[i].m == 0 ? got[i] != T(0) : !(d <= bound)) return false;
                }
                return true;
            };
            const bool ok = within(dda.get(), wa) && within(ddb.get(), wb);
            std::printf("%s %s%s softgrad %s\n", tag, name, f32 ? " f32" : "", ok ? "pass" : "error");
        }
    } catch (const std::exception&) {
        std::printf("%s %s%s %s error\n", tag, name, f32 ? " f32" : "", stage);
    }
}

// --batch NB: NB seeded value sets in one batched call on a plan of `width`, beside NB unbatched calls on a
// width-1 plan of the same type T; with check every set of the batched call against its reference (see the top).
// acc64 (T = float): both plans are mixed ones (FP64 sums), checked by acc64_within on C's host pattern.
template <class T>
static void run_batch(Tool& tools, const CSR& A, const CSR& B, const CSR& C, int calls, int nb, int width, bool check,
                      bool acc64 = false) {
    const bool f32 = sizeof(T) == sizeof(float);
    const char* tag = acc64 ? "batched f32 acc64" : f32 ? "batched f32" : "batched";
    const int acc = acc64 ? MHS_ACC_F64 : MHS_ACC_NATIVE;
    try {
        const size_t nA = (size_t)A.nnz, nB = (size_t)B.nnz, nC = (size_t)C.nnz, sets = (size_t)nb;
        unsigned long long state = 0x9e3779b97f4a7c15ULL;  // the seed
        auto seeded = [&](size_t n) {                       // in [0.1, 1), as T holds them
            std::vector<T> v(n);
            for (size_t i = 0; i < n; ++i) {
                state = state * 6364136223846793005ULL + 1442695040888963407ULL;
                v[i] = (T)(0.1 + 0.9 * (double)(state >> 11) / 9007199254740992.0);
            }
            return v;
        };
        const std::vector<T> va = seeded(sets * nA), vb = seeded(sets * nB);
        const mhs_dtype dt = f32 ? MHS_F32 : MHS_F64;
        mhs_shim::ValuesPlan wide(tools, A, B, C, false, MHS_MASK_PRODUCT, dt, width, MHS_SR_PLUS_TIMES, acc);
        mhs_shim::ValuesPlan one(tools, A, B, C, false, MHS_MASK_PRODUCT, dt, 1, MHS_SR_PLUS_TIMES, acc);
        DevArr<T> a(sets * nA), b(sets * nB), c(sets * nC), c1(sets * nC);
        a.put(va), b.put(vb);
        std::vector<double> tb, tl;
        for (int i = 0; i < calls; ++i) {
            MH_spgemm_values_batched(nb, a.p, (int64_t)nA, b.p, (int64_t)nB, c.p, (int64_t)nC, wide);
            tb.push_back(wide.last_ms);
        }
        for (int i = 0; i < calls; ++i) {
            double sum = 0;
            for (size_t k = 0; k < sets; ++k) {
                MH_spgemm_values_batched(1, a.p + k * nA, 0, b.p + k * nB, 0, c1.p + k * nC, 0, one);
                sum += one.last_ms;
            }
            tl.push_back(sum);
        }
        std::printf("MH-SpGEMM values batched %s (%d sets, width %d) median of %d calls is %.3lf ms, %d unbatched calls %.3lf ms\n",
                    acc64 ? "FP32, FP64 sums" : f32 ? "FP32" : "FP64", nb, width, calls, median(tb), nb, median(tl));
        if (check) {
            // FP64 calls on a width-1 plan: m per entry from all-ones, and per set the reference / S on the set's values
            mhs_shim::ValuesPlan p64(tools, A, B, C, false, MHS_MASK_PRODUCT, MHS_F64, 1);
            DevArr<double> da(nA), db(nB), dc(nC);
            da.put(std::vector<double>(nA, 1.0)), db.put(std::vector<double>(nB, 1.0));
            f32_ok(p64.ctx, mhs_spgemm_values(p64.ctx, p64.plan, da.p, db.p, dc.p, nullptr));
            const std::vector<double> m = dc.get();
            const std::vector<T> got = c.get();
            const double u = f32 ? 5.9604644775390625e-8 : 1.1102230246251565e-16, factor = f32 ? 1.01 : 2 * 1.01;
            bool ok = true;
            for (size_t k = 0; k < sets && ok; ++k) {
                da.put(std::vector<double>(va.begin() + k * nA, va.begin() + (k + 1) * nA));
                db.put(std::vector<double>(vb.begin() + k * nB, vb.begin() + (k + 1) * nB));
                f32_ok(p64.ctx, mhs_spgemm_values(p64.ctx, p64.plan, da.p, db.p, dc.p, nullptr));
                const std::vector<double> ref = dc.get();  // (positive values: also S)
                if constexpr (sizeof(T) == sizeof(float)) {
                    if (acc64) {
                        ok = acc64_within(C, width, wide.info().rows[6], false, got.data() + k * nC, ref, m, ref);
                        continue;
                    }
                }
                for (size_t i = 0; i < nC && ok; ++i) {
                    const double mm = std::floor(m[i] + 0.5), g = (double)got[k * nC + i];
                    ok = mm == 0 ? g == 0.0 : std::fabs(g - ref[i]) <= factor * mm * u * ref[i];
                }
            }
            std::printf("%s %s\n", tag, ok ? "pass" : "error");
        }
    } catch (const std::exception&) {
        std::printf("%s error\n", tag);
    }
}

// The unbatched backward on device arrays of either type (mhs_spgemm_values_grad / _f32)
static void grad_unbatched(mhs_shim::ValuesPlan& p, const double* a, const double* b, const double* g, double* da, double* db) {
    f32_ok(p.ctx, mhs_spgemm_values_grad(p.ctx, p.plan, a, b, g, da, db, &p.last_ms));
}
static void grad_unbatched(mhs_shim::ValuesPlan& p, const float* a, const float* b, const float* g, float* da, float* db) {
    f32_ok(p.ctx, mhs_spgemm_values_grad_f32(p.ctx, p.plan, a, b, g, da, db, &p.last_ms));
}

// --grad N with --batch NB: the backward of the batched call, NB seeded value and cotangent sets in one call of
// mhs_spgemm_values_grad_batched on a plan of `width`, beside NB unbatched backward calls on a width-1 plan of the
// same type T; with check every set of the batched call against the unbatched call on that set (see the top).
// acc64 (T = float): both plans are mixed ones; their backward is the float kernels', so the check is the FP32 one.
template <class T>
static void run_grad_batch(Tool& tools, const CSR& A, const CSR& B, const CSR& C, int calls, int nb, int width, bool check,
                           bool acc64 = false) {
    const bool f32 = sizeof(T) == sizeof(float);
    const char* tag = acc64 ? "grad batched f32 acc64" : f32 ? "grad batched f32" : "grad batched";
    const int acc = acc64 ? MHS_ACC_F64 : MHS_ACC_NATIVE;
    try {
        const size_t nA = (size_t)A.nnz, nB = (size_t)B.nnz, nC = (size_t)C.nnz, sets = (size_t)nb;
        unsigned long long state = 0x9e3779b97f4a7c15ULL;  // the seed
        auto seeded = [&](size_t n) {                       // in [0.1, 1), as T holds them
            std::vector<T> v(n);
            for (size_t i = 0; i < n; ++i) {
                state = state * 6364136223846793005ULL + 1442695040888963407ULL;
                v[i] = (T)(0.1 + 0.9 * (double)(state >> 11) / 9007199254740992.0);
            }
            return v;
        };
        const mhs_dtype dt = f32 ? MHS_F32 : MHS_F64;
        mhs_shim::ValuesPlan wide(tools, A, B, C, false, MHS_MASK_PRODUCT, dt, width, MHS_SR_PLUS_TIMES, acc);
        mhs_shim::ValuesPlan one(tools, A, B, C, false, MHS_MASK_PRODUCT, dt, 1, MHS_SR_PLUS_TIMES, acc);
        DevArr<T> a(sets * nA), b(sets * nB), g(sets * nC), da(sets * nA), db(sets * nB), da1(sets * nA), db1(sets * nB);
        a.put(seeded(sets * nA)), b.put(seeded(sets * nB)), g.put(seeded(sets * nC));
        std::vector<double> tb, tl;
        for (int i = 0; i < calls; ++i) {
            MH_spgemm_values_grad_batched(nb, a.p, (int64_t)nA, b.p, (int64_t)nB, g.p, (int64_t)nC, da.p, (int64_t)nA, db.p, (int64_t)nB,
                                          wide);
            tb.push_back(wide.last_ms);
        }
        for (int i = 0; i < calls; ++i) {
            double sum = 0;
            for (size_t k = 0; k < sets; ++k) {
                grad_unbatched(one, a.p + k * nA, b.p + k * nB, g.p + k * nC, da1.p + k * nA, db1.p + k * nB);
                sum += one.last_ms;
            }
            tl.push_back(sum);
        }
        std::printf("MH-SpGEMM values grad batched %s (%d sets, width %d) median of %d calls is %.3lf ms, %d unbatched calls %.3lf ms\n",
                    acc64 ? "FP32, FP64 sums" : f32 ? "FP32" : "FP64", nb, width, calls, median(tb), nb, median(tl));
        if (check) {
            // m per entry from the unbatched call on all-ones; the seeded values are positive, so a set's unbatched
            // result is also its S, and the two calls -- each within 1.01 m u S of the exact sum -- differ by at most twice that
            DevArr<T> ones_a(nA), ones_b(nB), ones_g(nC), ma(nA), mb(nB);
            ones_a.put(std::vector<T>(nA, (T)1)), ones_b.put(std::vector<T>(nB, (T)1)), ones_g.put(std::vector<T>(nC, (T)1));
            grad_unbatched(one, ones_a.p, ones_b.p, ones_g.p, ma.p, mb.p);
            const std::vector<T> mA = ma.get(), mB = mb.get(), gotA = da.get(), gotB = db.get(), refA = da1.get(), refB = db1.get();
            const double u = f32 ? 5.9604644775390625e-8 : 1.1102230246251565e-16;
            auto within = [&](const std::vector<T>& got, const std::vector<T>& ref, const std::vector<T>& m, size_t n) {
                for (size_t k = 0; k < sets; ++k)
                    for (size_t i = 0; i < n; ++i) {
                        const double mm = std::floor((double)m[i] + 0.5), x = (double)got[k * n + i], r = (double)ref[k * n + i];
                        if (mm == 0 ? x != 0.0 : !(std::fabs(x - r) <= 2 * 1.01 * mm * u * r)) return false;
                    }
                return true;
            };
            std::printf("%s %s\n", tag, within(gotA, refA, mA, nA) && within(gotB, refB, mB, nB) ? "pass" : "error");
        }
    } catch (const std::exception&) {
        std::printf("%s error\n", tag);
    }
}

int main(int argc, char** argv) {
    int iters = 1, warmup = 1, reuse = 0, masked = 0, grad = 0, batch = 0, width = 0, semiring = -1, subgrad = 0, witness = 0, softgrad = 0;
    bool smooth = false;
    bool has_semiring = false;
    bool aat = false, vendor = false, check = false, cache = false, f32 = false, acc64 = false;
    std::string csv;
    const char* filename = nullptr;
    bool bad = false;
    for (int i = 1; i < argc; ++i) {
        if (!std::strcmp(argv[i], "--iters") && i + 1 < argc) iters = std::atoi(argv[++i]);
        else if (!std::strcmp(argv[i], "--warmup") && i + 1 < argc) warmup = std::atoi(argv[++i]);
        else if (!std::strcmp(argv[i], "--aat")) aat = true;
        else if (!std::strcmp(argv[i], "--vendor")) vendor = true;
        else if (!std::strcmp(argv[i], "--check")) check = vendor = true;
        else if (!std::strcmp(argv[i], "--csv") && i + 1 < argc) csv = argv[++i];
        else if (!std::strcmp(argv[i], "--cache")) cache = true;
        else if (!std::strcmp(argv[i], "--reuse") && i + 1 < argc) reuse = std::atoi(argv[++i]);
        else if (!std::strcmp(argv[i], "--masked") && i + 1 < argc) masked = std::atoi(argv[++i]);
        else if (!std::strcmp(argv[i], "--grad") && i + 1 < argc) grad = std::atoi(argv[++i]);
        else if (!std::strcmp(argv[i], "--f32")) f32 = true;
        else if (!std::strcmp(argv[i], "--acc64")) acc64 = true;
        else if (!std::strcmp(argv[i], "--batch") && i + 1 < argc) batch = std::atoi(argv[++i]), bad = bad || batch < 1;
        else if (!std::strcmp(argv[i], "--width") && i + 1 < argc) {
            width = std::atoi(argv[++i]);
            bad = bad || !(width == 1 || width == 2 || width == 4);
        }
        else if (!std::strcmp(argv[i], "--semiring") && i + 1 < argc) {
            semiring = semiring_of(argv[++i]);
            has_semiring = true;
            bad = bad || semiring < 0;
        }
        else if (!std::strcmp(argv[i], "--subgrad") && i + 1 < argc) subgrad = std::atoi(argv[++i]), bad = bad || subgrad < 1;
        else if (!std::strcmp(argv[i], "--witness") && i + 1 < argc) witness = std::atoi(argv[++i]), bad = bad || witness < 1;
        else if (!std::strcmp(argv[i], "--smooth") && i + 1 < argc) smooth = true, bad = bad || std::strcmp(argv[++i], "lse") != 0;
        else if (!std::strcmp(argv[i], "--softgrad") && i + 1 < argc) softgrad = std::atoi(argv[++i]), bad = bad || softgrad < 1;
        else if (!filename && argv[i][0] != '-') filename = argv[i];
        else bad = true;
    }
    if (has_semiring && reuse <= 0 && masked <= 0) bad = true;  // (a modifier of --reuse and --masked)
    if ((subgrad > 0 || witness > 0) && (!has_semiring || semiring <= MHS_SR_PLUS_TIMES)) bad = true;  // (modifiers of --semiring, not plus_times)
    if (smooth && (!has_semiring || (semiring != MHS_SR_MIN_PLUS && semiring != MHS_SR_MAX_PLUS))) bad = true;  // (of --semiring min_plus | max_plus)
    if (softgrad > 0 && !smooth) bad = true;  // (a modifier of --smooth)
    if ((batch > 0 && reuse <= 0) || (width > 0 && batch <= 0)) bad = true;  // (modifiers of --reuse and of --batch)
    if (acc64 && !f32) bad = true;  // (a modifier of --f32)
    if (width == 0) width = MHS_VAL_WIDTH_MAX;
    if (bad || !filename || iters < 1 || warmup < 0 || reuse < 0 || masked < 0 || grad < 0) {
        std::puts("Invalid Arguments.");
        std::puts("Usage:\t ./spgemm [--iters K] [--warmup W] [--aat] [--vendor] [--check] [--csv DIR] [--cache] [--reuse N] [--masked N] [--grad N] [--f32] [--acc64] [--batch NB] [--width W] [--semiring NAME] [--subgrad N] [--witness N] [--smooth lse] [--softgrad N] <Input File>");
        return -1;
    }
    const std::string matrix_name = extract_matrix_name(filename);
    CSR A, B, C;
    if (readMtxFile(A, filename, cache) != 0) return -1;
    if (!aat && A.M != A.N) {
        std::puts("C=AA must have rowA = colA. Exit.");
        return 0;
    }
    std::printf("--------------------------SpGEMM Start!!!--------------------------\n");
    double Gflops = 0, Gflops_v = 0;
    bool shared_b = false;
    try {
        Tool tools;
        A.H2D();
        if (aat && !A.isSymmetric) {
            matrix_transposition(A, B, tools);  // device A^T; B's host arrays for the flop count
        } else {
            // B = A: share A's device arrays (C = A*A, or A*A^T of a symmetric A), no second copy
            B = A;
            B.d_ptr = A.d_ptr;
            B.d_col = A.d_col;
            B.d_val = A.d_val;
            shared_b = true;
        }
        const unsigned long long int_result = mhs_flop_count(A.nnz, A.col, B.ptr);
        std::printf("Matrix %s (%d , %d) nnz:%d\n", matrix_name.c_str(), A.M, B.N, A.nnz);
        std::printf("SpGEMM intermediate result = %lld\n", (long long)int_result);
        Timing timing, bench;
        for (int i = 0; i < warmup; ++i) {
            MH_spgemm(A, B, C, timing, tools);
            recycle(tools, C);
        }
        for (int i = 0; i < iters; ++i) {
            MH_spgemm(A, B, C, timing, tools);
            bench += timing;
            if (i < iters - 1) recycle(tools, C);
        }
        bench /= iters;
        bench.print_step_time();
        Gflops = 2.0 * (double)int_result / (bench.getTotal() * 1e6);
        std::printf("MH-SpGEMM runtime is %.3lfms, Gflops is %.2lf\n", bench.getTotal(), Gflops);
        std::printf("MH-SpGEMM e2e (incl. form_mask_matrix_B) is %.3lfms, Gflops is %.2lf\n", bench.total_e2e,
                    2.0 * (double)int_result / (bench.total_e2e * 1e6));
        if (vendor) {
            mhs_csr a{A.M, A.N, A.nnz, A.d_ptr, A.d_col, A.d_val};
            mhs_csr b{B.M, B.N, B.nnz, B.d_ptr, B.d_col, B.d_val};
            mhs_csr v{};
            double ms = 0;
            char err[256] = {0};
            // one untimed call first: rocSPARSE loads its code objects on first use
            int vrc = mhs_vendor_spgemm(0, &a, &b, &v, &ms, err, (int)sizeof err);
            if (vrc == MHS_OK) {
                mhs_vendor_free(&v);
                vrc = mhs_vendor_spgemm(0, &a, &b, &v, &ms, err, (int)sizeof err);
            }
            if (vrc == MHS_OK) {
                std::printf("rocSPARSE C.nnz = %d\n", v.nnz);
                Gflops_v = 2.0 * (double)int_result / (ms * 1e6);
                std::printf("rocsparse: %.3lfms, Gflops is %.2lf\n", ms, Gflops_v);
                if (check) {
                    CSR vc;
                    vc.M = v.M;
                    vc.N = v.N;
                    vc.nnz = v.nnz;
                    vc.d_ptr = v.ptr;
                    vc.d_col = v.col;
                    vc.d_val = v.val;
                    C.D2H();
                    vc.D2H();
                    try {
                        std::puts(C == vc ? "pass" : "error");
                    } catch (const std::exception&) {
                        std::puts("error");
                    }
                    vc.d_ptr = vc.d_col = nullptr;  // freed below by mhs_vendor_free
                    vc.d_val = nullptr;
                }
                mhs_vendor_free(&v);
            } else {
                std::printf("rocSPARSE failed!!! (%s)\n", err);
            }
        }
        if (reuse > 0) {
            CSR full;  // the product's own values, before the values calls overwrite C.d_val
            if (check) {
                C.D2H();
                full = C;
            }
            {
                mhs_shim::ValuesPlan plan(tools, A, B, C);
                double sum = 0;
                for (int i = 0; i < reuse; ++i) {
                    MH_spgemm_values(A, B, C, plan);
                    sum += plan.last_ms;
                }
                std::printf("MH-SpGEMM values-only (pattern reused) mean of %d calls is %.3lfms, Gflops is %.2lf\n", reuse,
                            sum / reuse, 2.0 * (double)int_result / (sum / reuse * 1e6));
            }
            if (check) {
                C.D2H();
                try {
                    std::puts(full == C ? "values pass" : "values error");
                } catch (const std::exception&) {
                    std::puts("values error");
                }
            }
        }
        if (masked > 0 && A.M != A.N) std::puts("masked: A's pattern as the mask must have rowA = colA. Skipped.");
        else if (masked > 0) run_masked(tools, A, B, C, masked, check);
        if (grad > 0) run_grad(tools, A, B, C, grad, check);
        if (f32) {
            if (acc64 && check) C.D2H();  // (the pattern's host arrays: the mixed forward's check picks out the global class)
            if (reuse > 0) run_f32(tools, A, B, C, false, false, reuse, check, "values-only (pattern reused)", "values");
            if (reuse > 0 && acc64) run_f32(tools, A, B, C, false, false, reuse, check, "values-only (pattern reused)", "values", true);
            if (masked > 0 && A.M == A.N) {
                CSR mask;  // A's pattern (a plan reads no values)
                const bool owns = mask_of(A, B.N, mask);
                run_f32(tools, A, B, mask, true, false, masked, check, "masked (A's pattern)", "masked");
                if (acc64) run_f32(tools, A, B, mask, true, false, masked, check, "masked (A's pattern)", "masked", true);
                unborrow_mask(mask, owns);
            }
            if (grad > 0) run_f32(tools, A, B, C, false, true, grad, check, "values backward (both gradients)", "grad");
            if (grad > 0 && acc64) run_f32(tools, A, B, C, false, true, grad, check, "values backward (both gradients)", "grad", true);
        }
        if (batch > 0) {
            run_batch<double>(tools, A, B, C, reuse, batch, width, check);
            if (f32) run_batch<float>(tools, A, B, C, reuse, batch, width, check);
            if (acc64) run_batch<float>(tools, A, B, C, reuse, batch, width, check, true);
            if (grad > 0) {
                run_grad_batch<double>(tools, A, B, C, grad, batch, width, check);
                if (f32) run_grad_batch<float>(tools, A, B, C, grad, batch, width, check);
                if (acc64) run_grad_batch<float>(tools, A, B, C, grad, batch, width, check, true);
            }
        }
        if (has_semiring) {
            if (reuse > 0) {
                C.D2H();  // (the pattern's host arrays)
                run_semiring<double>(tools, A, B, C, false, semiring, reuse, check, "values-only (pattern reused)", "values");
                if (subgrad > 0) run_subgrad<double>(tools, A, B, C, false, semiring, subgrad, check, "values-only (pattern reused)", "values");
                if (witness > 0) run_witness<double>(tools, A, B, C, false, semiring, witness, check, "values-only (pattern reused)", "values");
                if (f32) run_semiring<float>(tools, A, B, C, false, semiring, reuse, check, "values-only (pattern reused)", "values");
                if (f32 && subgrad > 0) run_subgrad<float>(tools, A, B, C, false, semiring, subgrad, check, "values-only (pattern reused)", "values");
                if (f32 && witness > 0) run_witness<float>(tools, A, B, C, false, semiring, witness, check, "values-only (pattern reused)", "values");
                if (smooth) run_soft<double>(tools, A, B, C, false, semiring, reuse, softgrad, check, "values-only (pattern reused)", "values");
                if (smooth && f32) run_soft<float>(tools, A, B, C, false, semiring, reuse, softgrad, check, "values-only (pattern reused)", "values");
            }
            if (masked > 0 && A.M == A.N) {
                CSR mask;  // A's pattern (a plan reads no values)
                const bool owns = mask_of(A, B.N, mask);
                run_semiring<double>(tools, A, B, mask, true, semiring, masked, check, "masked (A's pattern)", "masked");
                if (subgrad > 0) run_subgrad<double>(tools, A, B, mask, true, semiring, subgrad, check, "masked (A's pattern)", "masked");
                if (witness > 0) run_witness<double>(tools, A, B, mask, true, semiring, witness, check, "masked (A's pattern)", "masked");
                if (f32) run_semiring<float>(tools, A, B, mask, true, semiring, masked, check, "masked (A's pattern)", "masked");
                if (f32 && subgrad > 0) run_subgrad<float>(tools, A, B, mask, true, semiring, subgrad, check, "masked (A's pattern)", "masked");
                if (f32 && witness > 0) run_witness<float>(tools, A, B, mask, true, semiring, witness, check, "masked (A's pattern)", "masked");
                if (smooth) run_soft<double>(tools, A, B, mask, true, semiring, masked, softgrad, check, "masked (A's pattern)", "masked");
                if (smooth && f32) run_soft<float>(tools, A, B, mask, true, semiring, masked, softgrad, check, "masked (A's pattern)", "masked");
                unborrow_mask(mask, owns);
            }
        }
        C.d_release_csr();
    } catch (const std::exception&) {
        std::printf("MH-SpGEMM failed!!!\n");
        Gflops = 0;
    }
    if (shared_b) {  // A owns the device arrays
        B.d_ptr = B.d_col = nullptr;
        B.d_val = nullptr;
    }
    if (!csv.empty()) {
        append_csv(csv, "Gflops_MH-SpGEMM.csv", Gflops);
        if (vendor) append_csv(csv, "Gflops_rocsparse.csv", Gflops_v);
    }
    std::printf("--------------------------SpGEMM   End!!!--------------------------\n");
    return 0;
}
