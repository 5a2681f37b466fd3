// mh_spgemm.hpp -- header-only C++ shim over the C-ABI (mhspgemm.h) that gives
// a driver written against the reference the reference's own surface:
//
//   class CSR      (inc/CSR.h:4-44, src/CSR.cu:4-135)   host + device arrays,
//                  H2D / D2H, operator== (the cuSPARSE-style checker)
//   class Timing   (inc/Timing.h, src/Timing.cpp)       7 phase fields, getTotal()
//   class Tool     (inc/Tool.h, src/Tool.cu)            here: owns the mhs_ctx
//   void MH_spgemm(const CSR&, CSR&, CSR&, Timing&, Tool&)   (src/main.cu:12-72)
//   int  readMtxFile(CSR&, const char*)                      (inc/mmio_read.h:34)
// and, beyond the reference, the values-only call on a kept pattern:
//   class mhs_shim::ValuesPlan                               owns an mhs_values_plan
//   void MH_spgemm_values(const CSR&, const CSR&, CSR&, mhs_shim::ValuesPlan&)
//   void MH_spgemm_values_batched(nb, Aval, strideA, Bval, strideB, Cval, strideC, mhs_shim::ValuesPlan&)
//   void MH_spgemm_values_grad_batched(nb, Aval, strideA, Bval, strideB, dC, strideG, dA, strideDA, dB, strideDB,
//                                      mhs_shim::ValuesPlan&)
//
// Errors: the C-ABI returns codes; this shim rethrows as std::runtime_error so a
// caller's try { MH_spgemm(...) } catch (...) { "MH-SpGEMM failed!!!" } behaves as
// in the reference (src/main.cu:117-145).  B is not mutated (no d_tile* arrays).
#pragma once
#include <hip/hip_runtime.h>

#include <cassert>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>

#include "mhspgemm.h"

namespace mhs_shim {
inline void hip_check(hipError_t e, const char* what) {
    if (e != hipSuccess) {
        std::printf("%s in %s\n", hipGetErrorString(e), what);
        throw std::runtime_error(what);
    }
}
}  // namespace mhs_shim

class CSR {
public:
    int M = 0, N = 0, nnz = 0;
    int* ptr = nullptr;
    int* col = nullptr;
    double* val = nullptr;
    int* d_ptr = nullptr;
    int* d_col = nullptr;
    double* d_val = nullptr;
    int isSymmetric = 0;

    CSR() = default;
    CSR(const CSR&) = delete;
    ~CSR() { release(); }

    void alloc(int r, int c, int n) {
        h_release_csr();
        M = r;
        N = c;
        nnz = n;
        ptr = new int[r + 1]();
        col = new int[n > 0 ? n : 1];
        val = new double[n > 0 ? n : 1];
    }
    // deep host copy, as the reference (src/CSR.cu:34-47)
    CSR& operator=(const CSR& A) {
        if (this == &A) return *this;
        alloc(A.M, A.N, A.nnz);
        isSymmetric = A.isSymmetric;
        std::memcpy(ptr, A.ptr, sizeof(int) * (size_t)(M + 1));
        std::memcpy(col, A.col, sizeof(int) * (size_t)nnz);
        std::memcpy(val, A.val, sizeof(double) * (size_t)nnz);
        return *this;
    }
    // CSR::operator== (src/CSR.cu:48-96): nnz mismatch throws; ptr and col exact;
    // val accepted when |d| < 1e-9 or |d| < 1e-9 * |this->val|; > 10 errors throws.
    bool operator==(const CSR& o) const {
        if (nnz != o.nnz) {
            std::printf("nnz not equal %d %d\n", nnz, o.nnz);
            throw std::runtime_error("nnz not equal");
        }
        assert(M == o.M && N == o.N);
        int err = 0;
        const double eps = 1e-9;
        for (int i = 0; i < M; i++) {
            if (err > 10) throw std::runtime_error("matrix compare: error num exceed threshold");
            if (ptr[i] != o.ptr[i]) {
                std::printf("ptr not equal at %d rows, %d != %d\n", i, ptr[i], o.ptr[i]);
                err++;
            }
            for (int j = ptr[i]; j < ptr[i + 1]; j++) {
                if (err > 10) throw std::runtime_error("matrix compare: error num exceed threshold");
                if (col[j] != o.col[j]) {
                    std::printf("col not equal at %d rows, index %d != %d\n", i, col[j], o.col[j]);
                    err++;
                }
                const double d = std::fabs(val[j] - o.val[j]);
                if (!(d < eps || d < eps * std::fabs(val[j]))) {
                    std::printf("val not eqaul at %d rows, value %.18le != %.18le\n", i, val[j], o.val[j]);
                    err++;
                }
            }
        }
        if (ptr[M] != o.ptr[M]) {
            std::printf("ptr[M] not equal\n");
            throw std::runtime_error("matrix compare: error num exceed threshold");
        }
        return err == 0;
    }
    void H2D() {
        using mhs_shim::hip_check;
        hip_check(hipMalloc((void**)&d_ptr, sizeof(int) * (size_t)(M + 1)), "hipMalloc d_ptr");
        hip_check(hipMalloc((void**)&d_col, sizeof(int) * (size_t)(nnz > 0 ? nnz : 1)), "hipMalloc d_col");
        hip_check(hipMalloc((void**)&d_val, sizeof(double) * (size_t)(nnz > 0 ? nnz : 1)), "hipMalloc d_val");
        hip_check(hipMemcpy(d_ptr, ptr, sizeof(int) * (size_t)(M + 1), hipMemcpyHostToDevice), "H2D ptr");
        hip_check(hipMemcpy(d_col, col, sizeof(int) * (size_t)nnz, hipMemcpyHostToDevice), "H2D col");
        hip_check(hipMemcpy(d_val, val, sizeof(double) * (size_t)nnz, hipMemcpyHostToDevice), "H2D val");
    }
    void D2H() {
        using mhs_shim::hip_check;
        h_release_csr();
        ptr = new int[M + 1];
        col = new int[nnz > 0 ? nnz : 1];
        val = new double[nnz > 0 ? nnz : 1];
        hip_check(hipMemcpy(ptr, d_ptr, sizeof(int) * (size_t)(M + 1), hipMemcpyDeviceToHost), "D2H ptr");
        hip_check(hipMemcpy(col, d_col, sizeof(int) * (size_t)nnz, hipMemcpyDeviceToHost), "D2H col");
        hip_check(hipMemcpy(val, d_val, sizeof(double) * (size_t)nnz, hipMemcpyDeviceToHost), "D2H val");
    }
    void h_release_csr() {
        delete[] ptr;
        delete[] col;
        delete[] val;
        ptr = col = nullptr;
        val = nullptr;
    }
    void d_release_csr() {
        if (d_ptr) (void)hipFree(d_ptr);
        if (d_col) (void)hipFree(d_col);
        if (d_val) (void)hipFree(d_val);
        d_ptr = d_col = nullptr;
        d_val = nullptr;
    }
    void release() {
        h_release_csr();
        d_release_csr();
    }
};

class Timing {
public:
    double mem_alloc = 0, Form_mask_matrix_B = 0, Calculate_C_nnz = 0, Malloc_C_col_val = 0, Numeric = 0,
           symbolic_binning = 0, numeric_binning = 0;
    double total_e2e = 0;
    unsigned long long flop = 0;

    void operator+=(const Timing& t) {
        mem_alloc += t.mem_alloc;
        Form_mask_matrix_B += t.Form_mask_matrix_B;
        Calculate_C_nnz += t.Calculate_C_nnz;
        Malloc_C_col_val += t.Malloc_C_col_val;
        Numeric += t.Numeric;
        symbolic_binning += t.symbolic_binning;
        numeric_binning += t.numeric_binning;
        total_e2e += t.total_e2e;
    }
    void operator/=(double x) {
        mem_alloc /= x;
        Form_mask_matrix_B /= x;
        Calculate_C_nnz /= x;
        Malloc_C_col_val /= x;
        Numeric /= x;
        symbolic_binning /= x;
        numeric_binning /= x;
        total_e2e /= x;
    }
    void print_step_time() const {
        std::printf("  -------------time-------------\n");
        std::printf("    mem_alloc: \t\t%.3lfms\n", mem_alloc);
        std::printf("    form_mask_matrix_B: %.3lfms\n", Form_mask_matrix_B);
        std::printf("    symbolic_binning: \t%.3lfms\n", symbolic_binning);
        std::printf("    calculate_C_nnz: \t%.3lfms\n", Calculate_C_nnz);
        std::printf("    malloc_C_col_val: \t%.3lfms\n", Malloc_C_col_val);
        std::printf("    numeric_binning: \t%.3lfms\n", numeric_binning);
        std::printf("    numeric: \t\t%.3lfms\n", Numeric);
        std::printf("  ------------------------------\n");
    }
    // src/Timing.cpp:39-41: excludes Form_mask_matrix_B
    double getTotal() const {
        return Calculate_C_nnz + Malloc_C_col_val + Numeric + symbolic_binning + numeric_binning + mem_alloc;
    }
};

class Tool {
public:
    mhs_ctx* ctx = nullptr;
    explicit Tool(int device = 0) {
        if (mhs_ctx_create(&ctx, device) != MHS_OK) throw std::runtime_error("mhs_ctx_create failed");
    }
    Tool(const Tool&) = delete;
    ~Tool() { mhs_ctx_destroy(ctx); }
    // The reference allocates per call (src/Tool.cu:4-45); the context keeps its
    // workspace across calls, release() trims it.
    void allocate(const CSR&, const CSR&) {}
    void release() { mhs_ctx_trim(ctx); }
};

inline void MH_spgemm(const CSR& A, CSR& B, CSR& C, Timing& timing, Tool& tools) {
    mhs_csr a{A.M, A.N, A.nnz, A.d_ptr, A.d_col, A.d_val};
    mhs_csr b{B.M, B.N, B.nnz, B.d_ptr, B.d_col, B.d_val};
    mhs_csr c{};
    mhs_timing t{};
    const int rc = mhs_spgemm(tools.ctx, &a, &b, &c, &t);
    if (rc != MHS_OK) {
        std::printf("%s\n", mhs_last_error(tools.ctx));
        throw std::runtime_error(mhs_last_error(tools.ctx));
    }
    C.d_release_csr();
    C.M = c.M;
    C.N = c.N;
    C.nnz = c.nnz;
    C.d_ptr = c.ptr;
    C.d_col = c.col;
    C.d_val = c.val;
    std::printf("C.nnz = %d\n", C.nnz);
    timing.mem_alloc = t.mem_alloc;
    timing.Form_mask_matrix_B = t.Form_mask_matrix_B;
    timing.symbolic_binning = t.symbolic_binning;
    timing.Calculate_C_nnz = t.Calculate_C_nnz;
    timing.numeric_binning = t.numeric_binning;
    timing.Malloc_C_col_val = t.Malloc_C_col_val;
    timing.Numeric = t.Numeric;
    timing.total_e2e = t.total_e2e;
    timing.flop = t.flop;
}

namespace mhs_shim {
// A values plan over the patterns of A, B and C (mhs_values_plan_create): C.d_ptr / C.d_col hold a
// pattern containing the product's, normally C of MH_spgemm.  The six pattern arrays are borrowed:
// they stay alive and unchanged while the plan lives.  Throws where the C-ABI returns an error.
class ValuesPlan {
public:
    mhs_ctx* ctx = nullptr;
    mhs_values_plan* plan = nullptr;
    // masked: C's pattern is a mask, possibly smaller than the product's (mhs_values_plan_create_masked);
    // form: an mhs_mask_form
    ValuesPlan(Tool& tools, const CSR& A, const CSR& B, const CSR& C, bool masked = false, int form = MHS_MASK_AUTO)
        : ctx(tools.ctx) {
        mhs_csr a{A.M, A.N, A.nnz, A.d_ptr, A.d_col, A.d_val};
        mhs_csr b{B.M, B.N, B.nnz, B.d_ptr, B.d_col, B.d_val};
        mhs_csr c{C.M, C.N, C.nnz, C.d_ptr, C.d_col, C.d_val};
        const int rc = masked ? mhs_values_plan_create_masked(ctx, &a, &b, &c, form, &plan)
                              : mhs_values_plan_create(ctx, &a, &b, &c, &plan);
        if (rc != MHS_OK) {
            std::printf("%s\n", mhs_last_error(ctx));
            throw std::runtime_error(mhs_last_error(ctx));
        }
    }
    // The typed constructor (mhs_values_plan_create_typed): a plan for values of `dtype`, MHS_F64 or MHS_F32.
    // An MHS_F32 plan runs through the float overloads of MH_spgemm_values and MH_spgemm_values_grad.
    ValuesPlan(Tool& tools, const CSR& A, const CSR& B, const CSR& C, bool masked, int form, mhs_dtype dtype) : ctx(tools.ctx) {
        mhs_csr a{A.M, A.N, A.nnz, A.d_ptr, A.d_col, A.d_val};
        mhs_csr b{B.M, B.N, B.nnz, B.d_ptr, B.d_col, B.d_val};
        mhs_csr c{C.M, C.N, C.nnz, C.d_ptr, C.d_col, C.d_val};
        if (mhs_values_plan_create_typed(ctx, &a, &b, &c, masked ? 1 : 0, form, (int)dtype, &plan) != MHS_OK) {
            std::printf("%s\n", mhs_last_error(ctx));
            throw std::runtime_error(mhs_last_error(ctx));
        }
    }
    // The batched constructor (mhs_values_plan_create_batched): a plan of `width` (1, 2 or 4) value sets per walk,
    // for MH_spgemm_values_batched.  Width 1 is the typed constructor's plan.
    // semiring: an mhs_semiring (mhs_values_plan_create_semiring).  A plan of another one than MHS_SR_PLUS_TIMES has
    // width 1; MH_spgemm_values and MH_spgemm_values_batched run it, the backward calls throw the library's refusal.
    // accum: an mhs_accum (mhs_values_plan_create_accum).  MHS_ACC_F64 with MHS_F32 is a mixed plan -- float values,
    // double sums, the float overloads run it -- and is plus-times only; with MHS_F64 it is the plain FP64 plan.
    ValuesPlan(Tool& tools, const CSR& A, const CSR& B, const CSR& C, bool masked, int form, mhs_dtype dtype, int width,
               int semiring = MHS_SR_PLUS_TIMES, int accum = MHS_ACC_NATIVE, int smooth = MHS_SMOOTH_NONE)
        : ctx(tools.ctx) {
        mhs_csr a{A.M, A.N, A.nnz, A.d_ptr, A.d_col, A.d_val};
        mhs_csr b{B.M, B.N, B.nnz, B.d_ptr, B.d_col, B.d_val};
        mhs_csr c{C.M, C.N, C.nnz, C.d_ptr, C.d_col, C.d_val};
        if (semiring != MHS_SR_PLUS_TIMES && width != 1) throw std::runtime_error("ValuesPlan: a semiring plan has width 1");
        if (semiring != MHS_SR_PLUS_TIMES && accum != MHS_ACC_NATIVE)
            throw std::runtime_error("ValuesPlan: a semiring plan has no sum type (accum must be MHS_ACC_NATIVE)");
        // smooth: an mhs_smooth (mhs_values_plan_create_smooth).  MHS_SMOOTH_LSE on a min-plus or max-plus plan: its
        // reduce is log-sum-exp, MH_spgemm_values runs it, its backward is mhs_spgemm_values_softgrad.
        const int rc = smooth != MHS_SMOOTH_NONE
                           ? mhs_values_plan_create_smooth(ctx, &a, &b, &c, masked ? 1 : 0, form, (int)dtype, semiring, smooth, &plan)
                       : semiring != MHS_SR_PLUS_TIMES
                           ? mhs_values_plan_create_semiring(ctx, &a, &b, &c, masked ? 1 : 0, form, (int)dtype, semiring, &plan)
                       : accum != MHS_ACC_NATIVE
                           ? mhs_values_plan_create_accum(ctx, &a, &b, &c, masked ? 1 : 0, form, (int)dtype, width, accum, &plan)
                           : mhs_values_plan_create_batched(ctx, &a, &b, &c, masked ? 1 : 0, form, (int)dtype, width, &plan);
        if (rc != MHS_OK) {
            std::printf("%s\n", mhs_last_error(ctx));
            throw std::runtime_error(mhs_last_error(ctx));
        }
    }
    ValuesPlan(const ValuesPlan&) = delete;
    ValuesPlan& operator=(const ValuesPlan&) = delete;
    ~ValuesPlan() { mhs_values_plan_destroy(ctx, plan); }
    mhs_values_info info() const {
        mhs_values_info i{};
        mhs_values_plan_info(plan, &i);
        return i;
    }
    // the products that land in C's pattern (all of them unless the plan is masked)
    long long kept() const {
        int64_t k = 0;
        mhs_values_plan_kept(plan, &k);
        return (long long)k;
    }
    // the plan's value type
    mhs_dtype dtype() const {
        int d = MHS_F64;
        mhs_values_plan_dtype(plan, &d);
        return (mhs_dtype)d;
    }
    // the plan's width: the value sets one walk sums
    int width() const {
        int w = 1;
        mhs_values_plan_width(plan, &w);
        return w;
    }
    // the plan's sum type: MHS_ACC_F64 on a mixed plan (float values, double sums) only
    mhs_accum accum() const {
        int a = MHS_ACC_NATIVE;
        mhs_values_plan_accum(plan, &a);
        return (mhs_accum)a;
    }
    // the hipEvent time of the last MH_spgemm_values call through this plan (ms)
    double last_ms = 0;
};
}  // namespace mhs_shim

// C.d_val = the values of A * B at C's pattern, from A.d_val and B.d_val (mhs_spgemm_values); the
// patterns are the plan's.  Rethrows on error like MH_spgemm.
inline void MH_spgemm_values(const CSR& A, const CSR& B, CSR& C, mhs_shim::ValuesPlan& plan) {
    const int rc = mhs_spgemm_values(plan.ctx, plan.plan, A.d_val, B.d_val, C.d_val, &plan.last_ms);
    if (rc != MHS_OK) {
        std::printf("%s\n", mhs_last_error(plan.ctx));
        throw std::runtime_error(mhs_last_error(plan.ctx));
    }
}

// The backward of MH_spgemm_values (mhs_spgemm_values_grad): for the cotangent dC on C's pattern (device,
// nnz(C) doubles) the gradients of A.d_val into dA and of B.d_val into dB (device, nnz(A) / nnz(B) doubles;
// either nullptr: not computed).  The call's hipEvent time goes to plan.last_ms.
inline void MH_spgemm_values_grad(const CSR& A, const CSR& B, const double* dC, double* dA, double* dB,
                                  mhs_shim::ValuesPlan& plan) {
    const int rc = mhs_spgemm_values_grad(plan.ctx, plan.plan, A.d_val, B.d_val, dC, dA, dB, &plan.last_ms);
    if (rc != MHS_OK) {
        std::printf("%s\n", mhs_last_error(plan.ctx));
        throw std::runtime_error(mhs_last_error(plan.ctx));
    }
}

// The same two calls on an MHS_F32 plan (mhs_spgemm_values_f32, mhs_spgemm_values_grad_f32): the values are the
// caller's float arrays on the device -- nnz(A), nnz(B), nnz(C) entries -- as a CSR's d_val is double.
inline void MH_spgemm_values(const float* Aval, const float* Bval, float* Cval, mhs_shim::ValuesPlan& plan) {
    const int rc = mhs_spgemm_values_f32(plan.ctx, plan.plan, Aval, Bval, Cval, &plan.last_ms);
    if (rc != MHS_OK) {
        std::printf("%s\n", mhs_last_error(plan.ctx));
        throw std::runtime_error(mhs_last_error(plan.ctx));
    }
}
inline void MH_spgemm_values_grad(const float* Aval, const float* Bval, const float* dC, float* dA, float* dB,
                                  mhs_shim::ValuesPlan& plan) {
    const int rc = mhs_spgemm_values_grad_f32(plan.ctx, plan.plan, Aval, Bval, dC, dA, dB, &plan.last_ms);
    if (rc != MHS_OK) {
        std::printf("%s\n", mhs_last_error(plan.ctx));
        throw std::runtime_error(mhs_last_error(plan.ctx));
    }
}

// nb value sets in one call (mhs_spgemm_values_batched / _f32): set b reads Aval + b * strideA and
// Bval + b * strideB and writes Cval + b * strideC (device arrays, strides in elements; an input stride of 0: one
// array shared by all sets).  Any plan runs it; a plan of width W shares each walk of the patterns among W sets.
inline void MH_spgemm_values_batched(int nb, const double* Aval, int64_t strideA, const double* Bval, int64_t strideB,
                                     double* Cval, int64_t strideC, mhs_shim::ValuesPlan& plan) {
    const int rc = mhs_spgemm_values_batched(plan.ctx, plan.plan, nb, Aval, strideA, Bval, strideB, Cval, strideC, &plan.last_ms);
    if (rc != MHS_OK) {
        std::printf("%s\n", mhs_last_error(plan.ctx));
        throw std::runtime_error(mhs_last_error(plan.ctx));
    }
}
inline void MH_spgemm_values_batched(int nb, const float* Aval, int64_t strideA, const float* Bval, int64_t strideB, float* Cval,
                                     int64_t strideC, mhs_shim::ValuesPlan& plan) {
    const int rc =
        mhs_spgemm_values_batched_f32(plan.ctx, plan.plan, nb, Aval, strideA, Bval, strideB, Cval, strideC, &plan.last_ms);
    if (rc != MHS_OK) {
        std::printf("%s\n", mhs_last_error(plan.ctx));
        throw std::runtime_error(mhs_last_error(plan.ctx));
    }
}

// The backward of MH_spgemm_values_batched (mhs_spgemm_values_grad_batched / _f32), on a plan of any width: set b
// reads Aval + b * strideA, Bval + b * strideB and the cotangent dC + b * strideG and writes dA + b * strideDA and
// dB + b * strideDB (either output nullptr: not computed, and the other operand's values are then not read).
// Gradients come back per set: strideG, strideDA and strideDB are at least nnz(C), nnz(A) and nnz(B) when nb > 1.
inline void MH_spgemm_values_grad_batched(int nb, const double* Aval, int64_t strideA, const double* Bval, int64_t strideB,
                                          const double* dC, int64_t strideG, double* dA, int64_t strideDA, double* dB,
                                          int64_t strideDB, mhs_shim::ValuesPlan& plan) {
    const int rc = mhs_spgemm_values_grad_batched(plan.ctx, plan.plan, nb, Aval, strideA, Bval, strideB, dC, strideG, dA, strideDA,
                                                  dB, strideDB, &plan.last_ms);
    if (rc != MHS_OK) {
        std::printf("%s\n", mhs_last_error(plan.ctx));
        throw std::runtime_error(mhs_last_error(plan.ctx));
    }
}
inline void MH_spgemm_values_grad_batched(int nb, const float* Aval, int64_t strideA, const float* Bval, int64_t strideB,
                                          const float* dC, int64_t strideG, float* dA, int64_t strideDA, float* dB,
                                          int64_t strideDB, mhs_shim::ValuesPlan& plan) {
    const int rc = mhs_spgemm_values_grad_batched_f32(plan.ctx, plan.plan, nb, Aval, strideA, Bval, strideB, dC, strideG, dA,
                                                      strideDA, dB, strideDB, &plan.last_ms);
    if (rc != MHS_OK) {
        std::printf("%s\n", mhs_last_error(plan.ctx));
        throw std::runtime_error(mhs_last_error(plan.ctx));
    }
}

// src/utils.cpp:20-46 (B = A^T for AAT, src/main.cu:98-99) on the device: A must be
// device-resident; B gets device arrays (and host arrays, as the reference's B).
inline void matrix_transposition(const CSR& A, CSR& B, Tool& tools) {
    mhs_csr a{A.M, A.N, A.nnz, A.d_ptr, A.d_col, A.d_val};
    mhs_csr t{};
    if (mhs_transpose(tools.ctx, &a, &t) != MHS_OK) throw std::runtime_error(mhs_last_error(tools.ctx));
    B.release();
    B.M = t.M;
    B.N = t.N;
    B.nnz = t.nnz;
    B.isSymmetric = 0;
    B.d_ptr = t.ptr;
    B.d_col = t.col;
    B.d_val = t.val;
    B.D2H();
}

// cache = true: a binary CSR cache beside the file (mhs_read_mtx_cached), re-parsed
// only when the .mtx changes.
inline int readMtxFile(CSR& A, const char* filename, bool cache = false) {
    mhs_host_csr h{};
    const int rc = cache ? mhs_read_mtx_cached(filename, nullptr, &h, nullptr) : mhs_read_mtx(filename, &h);
    if (rc != MHS_OK) {
        std::printf("Could not read Matrix Market file %s.\n", filename);
        return -1;
    }
    A.alloc(h.M, h.N, h.nnz);
    A.isSymmetric = h.is_symmetric;
    std::memcpy(A.ptr, h.ptr, sizeof(int) * (size_t)(h.M + 1));
    std::memcpy(A.col, h.col, sizeof(int) * (size_t)h.nnz);
    std::memcpy(A.val, h.val, sizeof(double) * (size_t)h.nnz);
    mhs_host_csr_free(&h);
    return 0;
}
