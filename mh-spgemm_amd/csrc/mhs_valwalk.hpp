// mhs_valwalk.hpp -- what the values kernels (mhs_values.hip, and mhs_values_mixed.hip, which is that file once
// more), the smoothed plans' kernels (mhs_values_smooth.hip), the three backwards (mhs_values_grad.hip,
// mhs_values_subgrad.hip and the second half of mhs_values_smooth.hip, through mhs_backwalk.hpp, which holds their
// walk) and the host side (mhs_values_api.cpp) share.  First the declarations: the argument structs and
// the launchers.  Then the device helpers of the forward and the backward walk: the wave-level LDS
// ordering point, the slot search, the XCD stretch of a block's list, the row frame (a class row's C
// segment, guarded against the launch's LDS region), the stage of A entries that the wave and block
// walks read their B rows from, the forward's walk over a row's products, and the kernel of a launch.
#pragma once
#include "mhs_internal.hpp"
#include "mhs_semiring.hpp"
#include "mhs_valplan.hpp"

#include <initializer_list>

namespace mhs {

// ---------------------------------------------------------- declarations ---
// The six pattern arrays a values plan borrows ...
struct ValPattern {
    int M;
    const int *Aptr, *Acol, *Bptr, *Bcol, *Cptr, *Ccol;
};
// ... and what a hot call's kernels take: each matrix as its pattern and the call's value array for it.
// V is the plan's value type, double or float: the type of every value array of a call, and -- but for the forward
// of a mixed plan (mhs_values_plan_create_accum), whose kernels take an accumulator type beside it -- of the LDS sums
// and of the atomics.
template <class V>
struct ValCsr {
    const int *ptr, *col;
    V* val;
};
// A batched call (mhs_spgemm_values_batched) runs the launch list once per pass of up to W value sets, W the
// plan's width: set w of the pass reads A.val + w * sA and B.val + w * sB and writes C.val + w * sC (strides in
// elements, 64-bit; 0: the one array shared by all sets), and only the sets w < nw exist -- the others' addresses
// lie outside the caller's arrays.  The unbatched call is nw = 1.
template <class V>
struct ValArgs {
    using Value = V;
    ValCsr<const V> A, B;
    ValCsr<V> C;
    long long sA = 0, sB = 0, sC = 0;
    int nw = 1;
};
// The products of one B entry with a staged A entry, one per set of the pass (V: the forward's accumulator type)
template <class V, int W>
struct ValSums {
    V x[W];
};
// The backward's (mhs_spgemm_values_grad).  C.val is G, the cotangent on C's pattern; dA / dB: the gradients,
// zero-filled by the caller, either nullptr (that side is not computed, and B.val / A.val is then not read).
// A batched backward (mhs_spgemm_values_grad_batched) runs the launch list once per pass of up to W sets, as the
// forward does: set w of the pass reads A.val + w * sA, B.val + w * sB (0: shared) and the cotangent C.val + w * sG
// and writes dA + w * sDA and dB + w * sDB (strides in elements, 64-bit); only the sets w < nw exist.  The unbatched
// call is nw = 1, and a W = 1 kernel reads no stride.
template <class V>
struct ValGradArgs {
    using Value = V;
    ValCsr<const V> A, B, C;
    V *dA, *dB;
    long long sA = 0, sB = 0, sG = 0, sDA = 0, sDB = 0;
    int nw = 1;
};
// A masked plan's B^T pattern (transpose_pattern of B), read by the dot class only; tptr null: none
struct ValTrans {
    const int *tptr, *trow, *tperm;
};
// How a masked plan classifies: the form (ValMaskForm), AUTO's ratio, and B^T's row pointer for the dot cost
struct ValMask {
    const int* tptr;
    int form, ratio;
};
// Plan creation.  bad: a device int holding the first offending row (atomicMin; INT_MAX: none).
void launch_val_check_ptr(const int* ptr, int M, int nnz, int* bad, hipStream_t s);
void launch_val_check_cols(const int* ptr, const int* col, int M, int ncols, bool strict, int* bad, hipStream_t s);
// cnt: the counter block of mhs_valplan.hpp (VAL_CNT_INTS ints), zeroed by the caller; lists: M ints,
// class c's rows at the prefix of the counts before it; vb: the bytes of the plan's value type
void launch_val_classify(const ValPattern& p, int vb, int* cnt, int* lists, hipStream_t s);
void launch_val_verify(const ValPattern& p, int* bad, hipStream_t s);
// Masked plans: the same two classify passes by val_class_masked, and in place of the verify walk a
// count of the products that land in the mask, into the counter block's kept count
void launch_val_classify_masked(const ValPattern& p, const ValMask& m, int vb, int* cnt, int* lists, hipStream_t s);
void launch_val_count_kept(const ValPattern& p, int* cnt, hipStream_t s);
// One launch of a values plan (plan_values) over its class's row list, on `s` (t: read by VK_DOT only).
// V (double or float, both instantiated in mhs_values.hip) and `width` (1, 2 or 4) must be the type and the
// width the plan was classified for: the kernels' slice guards are taken at width x sizeof(V).  `semiring`
// (ValSemiring) is the plan's: SR_PLUS_TIMES at any width, the others at width 1 only.  `accum` (ValAccum) is the
// plan's sum type: VAL_ACC_F64 with V = float runs the mixed kernels, whose guards are taken at width x 8, on a
// plus-times plan; with V = double it is VAL_ACC_NATIVE.
template <class V>
void issue_values(const ValLaunch& l, int width, int semiring, int accum, const ValArgs<V>& a, const ValTrans& t,
                  const int* list, hipStream_t s);
// The mixed plans' part of the forward (mhs_values_mixed.hip): the attributes of its kernels (called by
// init_values_attributes), and one launch of an LDS class or of the dot class of a mixed plan of `width` -- issue_values
// hands them on; VK_GLOBAL is not among them.
hipError_t init_values_mixed_attributes();
void issue_values_mixed(const ValLaunch& l, int width, const ValArgs<float>& a, const ValTrans& t, const int* list,
                        hipStream_t s);
// One launch of a values plan's backward (plan_grad) over its class's row list, on `s` (mhs_values_grad.hip).
// V and `width` as for issue_values: the backward's kernels hold `width` cotangents per C entry where the
// forward's hold as many sums, behind the same slice guards.
template <class V>
void issue_values_grad(const ValLaunch& l, int width, const ValGradArgs<V>& a, const int* list, hipStream_t s);
hipError_t init_values_grad_attributes();  // (called by init_values_attributes)
// The subgradient's (mhs_spgemm_values_subgrad, a plan of min-plus, max-plus or max-min; mhs_values_subgrad.hip).
// C.val is Cval, the forward's result for (A.val, B.val); G the cotangent on C's pattern; ties: nnz(C) ints, the
// winners per C entry -- zero-filled by the caller, counted by pass 1, read by pass 2.  dA / dB: the gradients,
// zero-filled by the caller, either nullptr (that side is not computed); the winner test reads both operands always.
// wit: the witness's output (mhs_spgemm_values_witness, pass 3), nnz(C) ints filled with -1 by the caller; G, ties,
// dA and dB are nullptr in that pass, and wit in passes 1 and 2.
template <class V>
struct ValSubArgs {
    using Value = V;
    ValCsr<const V> A, B, C;
    const V* G;
    int* ties;
    V *dA, *dB;
    int* wit;
};
// One launch of a semiring plan's subgradient over its class's row list, on `s`: a launch of the plan's backward
// list (plan_grad) at width 1, run by its class's subgradient kernel for `semiring` (not SR_PLUS_TIMES: nothing is
// launched) and `pass` -- 1: every winner adds 1 to its entry of ties; 2: every winner carries G / ties to dA and dB;
// 3 (the witness): every winner takes the unsigned minimum of its inner index into its entry of wit.
template <class V>
void issue_values_subgrad(const ValLaunch& l, int semiring, int pass, const ValSubArgs<V>& a, const int* list, hipStream_t s);
hipError_t init_values_subgrad_attributes();  // (called by init_values_attributes)
// The smoothed plans' (mhs_values_plan_create_smooth, a min-plus or max-plus plan whose reduce is log-sum-exp;
// mhs_values_smooth.hip).  One launch of such a plan's forward (plan_values at twice the value's bytes: a max plane and
// a sum plane per C entry, laid out as a width-2 plan's) over its class's row list, on `s`; `semiring` is SR_MIN_PLUS
// or SR_MAX_PLUS (another: nothing is launched), t is read by VK_DOT only, a.nw is 1.
template <class V>
void issue_values_smooth(const ValLaunch& l, int semiring, const ValArgs<V>& a, const ValTrans& t, const int* list, hipStream_t s);
// Its gradient's (mhs_spgemm_values_softgrad).  C.val is Cval, the forward's result for (A.val, B.val); G the cotangent
// on C's pattern; dA / dB: the gradients, zero-filled by the caller, either nullptr (that side is not computed); both
// operands are read always.  sg: the sign of the plan's products (val_smooth_sign), set by issue_values_softgrad.
template <class V>
struct ValSoftArgs {
    using Value = V;
    ValCsr<const V> A, B, C;
    const V* G;
    V *dA, *dB;
    V sg;
};
// One launch of the gradient over its class's row list, on `s`: a launch of the plan's backward list (plan_grad at
// twice the value's bytes), the two planes holding G and Cval.
template <class V>
void issue_values_softgrad(const ValLaunch& l, int semiring, const ValSoftArgs<V>& a, const int* list, hipStream_t s);
hipError_t init_values_smooth_attributes();  // (called by init_values_attributes)

// -------------------------------------------------------- device helpers ---
// Ordering point for LDS traffic between lanes of one wave (a wave's LDS operations are
// performed in issue order; only the compiler must not move accesses across it).
static __device__ __forceinline__ void vwave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The policy of a value kernel: the plan's semiring (mhs_semiring.hpp: identity, mul, reg) with the reduce of one
// product into an LDS sum (lds: workgroup scope) and into the row's Cval segment (glob: the global class, agent
// scope), both relaxed and without a return value.  Plus-times: ds_add_f64 / ds_add_f32 and global_atomic_add_f64 /
// _f32, as before there was a policy.  min and max: ds_min_f64 / ds_max_f64 / ds_min_f32 / ds_max_f32 in LDS and
// global_atomic_min_f64 / _max_f64 in memory; gfx950 has no float min / max in global memory, so the FP32 global
// class reduces by a compare-and-swap loop.
template <int SR>
struct SrPolicy : SrValue<SR> {
    template <class V>
    static __device__ __forceinline__ void lds(V* p, V v) {
        if constexpr (SR == SR_PLUS_TIMES) atomicAdd(p, v);
        else if constexpr (SR == SR_MIN_PLUS) (void)__hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        else (void)__hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    template <class V>
    static __device__ __forceinline__ void glob(V* p, V v) {
        if constexpr (SR == SR_PLUS_TIMES) unsafeAtomicAdd(p, v);
        else if constexpr (SR == SR_MIN_PLUS) (void)__hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else (void)__hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
};
using PlusTimes = SrPolicy<SR_PLUS_TIMES>;  // the default of every kernel template: existing call sites read as before

// Position of column c in the ascending cols[0, n), or -1.
static __device__ __forceinline__ int find_slot(const int* cols, int n, int c) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (cols[mid] < c) lo = mid + 1;
        else hi = mid;
    }
    return lo < n && cols[lo] == c ? lo : -1;
}

// The list positions of a block-per-row kernel's block: begin, begin + step, ... below end.
// Consecutive rows read the same B rows, and blocks go to the 8 XCDs in turn: XCD x (blocks x, x + 8, ...)
// walks its own stretch of the list, in proportion to its blocks, so neighbours meet in one L2.
struct XcdStretch {
    int begin, end, step;
};
static __device__ __forceinline__ XcdStretch xcd_stretch(int count) {
    int lo = 0, hi = count, first = blockIdx.x, step = gridDim.x;
    if (gridDim.x >= 8) {
        const int xcd = blockIdx.x & 7;
        int before = 0;
        for (int y = 0; y < xcd; ++y) before += (gridDim.x - y + 7) >> 3;
        step = (gridDim.x - xcd + 7) >> 3;
        first = blockIdx.x >> 3;
        lo = (int)((long long)count * before / gridDim.x);
        hi = (int)((long long)count * (before + step) / gridDim.x);
    }
    return {lo + first, hi, step};
}

// The row frame of the LDS classes.  A row's LDS slice is `region` bytes: span-indexed sums of V (direct), or
// val_slice_entries sums and as many columns behind them (search).  The guards -- val_slice_entries and
// val_slice_fits of mhs_valplan.hpp, at W * sizeof(V), W the sets a walk sums (the backward: the cotangent sets it
// holds) -- are all that stands between a pattern that is not the plan's and an overrun of the slice: such a row is
// left alone.  W > 1: the sums (the backward: the cotangents) are set-major, val[w * pitch + slot] with pitch = span
// (direct) or ne (search), and the one column array lies behind all W planes.
template <class V>
struct ValSlice {
    V* val;
    int* cols;  // (search)
    int ne;     // entries the slice holds (search): the pitch of its sum planes
};
template <class V, int W = 1>
static __device__ __forceinline__ ValSlice<V> search_slice(char* base, int region) {
    const int ne = val_slice_entries(region, W * (int)sizeof(V));
    return {(V*)base, (int*)((V*)base + (size_t)W * ne), ne};
}
// A wave's or a block's row: body(s, n, first, span, val, cols) for C's segment [s, s + n) of `row`,
// when it has entries and fits (direct: columns first .. first + span - 1; search: first = span = 0).
// Acc: the type of the slice's sums where it is not the arguments' value type (void: it is) -- the forward of a
// mixed plan, double sums of float values; the guards are then taken at W * sizeof(Acc), as the plan classified.
template <class Acc, class Args>
struct ValAccOf {
    using type = Acc;
};
template <class Args>
struct ValAccOf<void, Args> {
    using type = typename Args::Value;
};
template <bool DIRECT, int W = 1, class Acc = void, class Args, class Body>
__device__ __forceinline__ void val_row(const Args& p, int row, char* base, int region, Body body) {
    using V = typename ValAccOf<Acc, Args>::type;
    const int s = p.C.ptr[row], n = p.C.ptr[row + 1] - s;
    if (n <= 0) return;
    if constexpr (DIRECT) {
        const int first = p.C.col[s];
        const long long span = (long long)p.C.col[s + n - 1] - first + 1;
        if (!val_slice_fits(span, region, W * (int)sizeof(V))) return;
        body(s, n, first, (int)span, (V*)base, (int*)nullptr);
    } else {
        const ValSlice<V> sl = search_slice<V, W>(base, region);
        if (n > sl.ne) return;
        body(s, n, 0, 0, sl.val, sl.cols);
    }
}
// A team's row: position idx of the list (-1 past its end), C's segment in s and n (n = 0: nothing to do).
template <class Args>
__device__ __forceinline__ int val_team_row(const Args& p, const int* list, int count, int idx, int ne, int& s, int& n) {
    const int row = idx < count ? list[idx] : -1;
    s = n = 0;
    if (row >= 0) {
        s = p.C.ptr[row];
        n = p.C.ptr[row + 1] - s;
        if (n > ne) n = 0;
    }
    return row;
}

// Up to CH staged A entries of a row as (B row start, length, A value); entry e of the stage that
// began at A position k0 is A entry k0 + e.  16 B an entry in FP64, 12 B in FP32.  A walk of W > 1 sets stages
// no A value: it reads each set's from A.val at the entry's position, beside the B loads (8 B an entry).
template <int CH, class V, int W = 1>
struct ValStage {
    int bs[CH], len[CH];
};
template <int CH, class V>
struct ValStage<CH, V, 1> {
    int bs[CH], len[CH];
    V av[CH];
};
static_assert(sizeof(ValStage<VAL_STAGE, double>) <= VAL_STAGE_BYTES && sizeof(ValStage<VAL_STAGE, float>) <= VAL_STAGE_BYTES &&
                  sizeof(ValStage<64, double>) <= 1024 && sizeof(ValStage<64, float>) <= 1024 &&
                  sizeof(ValStage<VAL_STAGE, double, VAL_WIDTH_MAX>) <= VAL_STAGE_BYTES && sizeof(ValStage<64, double, 2>) <= 1024,
              "the stage: VAL_STAGE_BYTES per block, 1 KiB per wave");
constexpr int VAL_PIECES = 8;  // G-wide pieces of a B row a lane group loads before its first sum
// ... of a walk of W sets: W values a piece, so the values in flight (and their registers) stay VAL_PIECES
constexpr int val_pieces(int W) { return VAL_PIECES / W; }
static_assert(val_pieces(1) == VAL_PIECES && val_pieces(VAL_WIDTH_MAX) >= 1, "W = 1 keeps its pieces; the widest walk has one");

// ----------------------------------------------------------- forward walk ---
// The products of row `row`: group g of ng groups takes A entries g, g + ng, ...; its G lanes
// stride over the B row.  add(column, value) per product.
// W: the plan's width.  The pattern work of a product -- the B column and, in add, its slot -- is done
// once, the value work for each of the pass's sets: add(column, sums) with sums.x[w] the product of set
// w < val_nw (set w's values lie w strides on: ValArgs); the x of a set the pass has not is not set.
template <int W, class V>
__device__ __forceinline__ int val_nw(const ValArgs<V>& a) {
    return W == 1 ? 1 : a.nw;
}
template <int G, int W, class S = PlusTimes, class Acc = void, class V, class F>
__device__ __forceinline__ void walk_products(const ValArgs<V>& a, int row, int g, int ng, int t, F add) {
    using Sum = typename ValAccOf<Acc, ValArgs<V>>::type;
    const int nw = val_nw<W>(a);
    const int ae = a.A.ptr[row + 1];
    for (int k = a.A.ptr[row] + g; k < ae; k += ng) {
        const int ac = a.A.col[k];
        V av[W];
#pragma unroll
        for (int w = 0; w < W; ++w)
            if (w < nw) av[w] = a.A.val[(long long)w * a.sA + k];
        const int be = a.B.ptr[ac + 1];
        for (int j = a.B.ptr[ac] + t; j < be; j += G) {
            const int c = a.B.col[j];
            ValSums<Sum, W> p;
#pragma unroll
            for (int w = 0; w < W; ++w)
                if (w < nw) p.x[w] = S::mul(Sum(av[w]), Sum(a.B.val[(long long)w * a.sB + j]));
            add(c, p);
        }
    }
}
// The same products for a wave's or a block's row, with memory-level parallelism: the row's `lanes`
// lanes first stage up to CH of its A entries as (B row start, length, A value) in LDS -- one
// dependent load chain (A.col -> B.ptr) per CH entries, not one per entry -- then each group of G
// lanes takes staged entries g, g + ng, ... and reads its B row VAL_PIECES G-wide pieces at a time,
// every load issued before the first sum.  pre() runs once, between the first stage's loads and the
// sync that publishes them (the row's zero fill rides on that sync).
// W > 1: the stage holds no A value (ValStage); a group reads each set's at the entry's A position, and
// val_pieces(W) pieces of W values each are in flight.
template <int G, int W, class S = PlusTimes, class Acc = void, int CH, class V, class Sync, class Pre, class F>
__device__ __forceinline__ void walk_staged(const ValArgs<V>& a, int row, int t, int lanes, ValStage<CH, V, W>& d, Sync sync,
                                            Pre pre, F add) {
    using Sum = typename ValAccOf<Acc, ValArgs<V>>::type;
    constexpr int P = val_pieces(W);
    const int nw = val_nw<W>(a);
    const int g = t / G, ng = lanes / G, tl = t % G;
    const int ae = a.A.ptr[row + 1], a0 = a.A.ptr[row];
    if (a0 >= ae) {
        pre();
        sync();
        return;
    }
    for (int k0 = a0; k0 < ae; k0 += CH) {
        const int cnt = ae - k0 < CH ? ae - k0 : CH;
        if (t < cnt) {
            const int ac = a.A.col[k0 + t];
            const int bs = a.B.ptr[ac];
            d.bs[t] = bs;
            d.len[t] = a.B.ptr[ac + 1] - bs;
            if constexpr (W == 1) d.av[t] = a.A.val[k0 + t];
        }
        if (k0 == a0) pre();
        sync();
        for (int e = g; e < cnt; e += ng) {
            const int bs = d.bs[e], len = d.len[e];
            V av[W];
            if constexpr (W == 1) {
                av[0] = d.av[e];
            } else {
#pragma unroll
                for (int w = 0; w < W; ++w)
                    if (w < nw) av[w] = a.A.val[(long long)w * a.sA + (k0 + e)];
            }
            for (int j = tl; j < len; j += P * G) {
                int c[P];
                V v[P][W];
#pragma unroll
                for (int u = 0; u < P; ++u) {
                    const int jj = j + u * G;
                    const bool in = jj < len;
                    c[u] = in ? a.B.col[bs + jj] : -1;
#pragma unroll
                    for (int w = 0; w < W; ++w)
                        if (w < nw) v[u][w] = in ? a.B.val[(long long)w * a.sB + (bs + jj)] : V(0);
                }
#pragma unroll
                for (int u = 0; u < P; ++u)
                    if (c[u] >= 0) {
                        ValSums<Sum, W> p;
#pragma unroll
                        for (int w = 0; w < W; ++w)
                            if (w < nw) p.x[w] = S::mul(Sum(av[w]), Sum(v[u][w]));
                        add(c[u], p);
                    }
            }
        }
        sync();
    }
}

// ---------------------------------------------------------------- launch ---
// The kernel of a launch over an LDS class's list, nullptr for the other kernels.  K names a direction's
// kernels: K::Fn, K::team(), K::wave<DIRECT>(), K::block<T, DIRECT>().
template <class K>
typename K::Fn val_lds_kernel(int kernel, int block) {
    const bool big = block == 1024;
    switch (kernel) {
    case VK_TEAM: return K::team();
    case VK_WAVE_DIRECT: return K::template wave<true>();
    case VK_WAVE_SEARCH: return K::template wave<false>();
    case VK_BLOCK_DIRECT: return big ? K::template block<1024, true>() : K::template block<256, true>();
    case VK_BLOCK_SEARCH: return big ? K::template block<1024, false>() : K::template block<256, false>();
    default: return nullptr;
    }
}
// The 1024-thread block kernels may take the whole 160 KiB (the 256-thread ones run at most VAL_BLOCK_SMALL).
template <class K>
hipError_t val_allow_max_lds() {
    for (int kernel : {VK_BLOCK_DIRECT, VK_BLOCK_SEARCH}) {
        const hipError_t e = hipFuncSetAttribute((const void*)val_lds_kernel<K>(kernel, 1024),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, VAL_BLOCK_BYTES);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace mhs
