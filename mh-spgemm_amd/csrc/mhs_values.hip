// mhs_values.hip -- values-only SpGEMM: recompute C.val on a kept pattern (mhs_spgemm_values).
//
// Plan creation (once per pattern): k_val_check_ptr and k_val_check_cols validate the three
// patterns, k_val_classify puts every row of C into its class list (mhs_valplan.hpp),
// k_val_verify walks every product's column once and looks it up in its C row.
// Hot call: one value kernel per non-empty class.  Each walks A's row, then B's rows, reads
// Aval / Bval only for values, and -- told the row's sorted columns -- only finds each product's
// slot: by subtraction (direct classes) or by binary search (team, search and global classes).
// Every value kernel is a template on the plan's value type V (double or float: ValArgs<V>) and on its width
// W (1, 2 or 4: the value sets one walk sums, mhs_spgemm_values_batched; W = 1 is the unbatched kernel); sums are
// atomics of that type: ds_add_f64 / ds_add_f32 in LDS, global_atomic_add_f64 / _f32 in the global class.
// Masked plans (mhs_values_plan_create_masked: C's pattern is a mask, products outside it are dropped)
// classify by val_class_masked, count the kept products in place of the verify walk, and may send rows
// to the dot class: k_val_dot, the inner-product form over B^T's pattern (no sums shared, no atomics).
// The algebra is a policy S (SrPolicy of mhs_valwalk.hpp over mhs_semiring.hpp), the last template parameter of the
// walks and the value kernels: S::identity() in the fills, S::mul for a product, S::lds / S::glob for the reduce of a
// product into an LDS or a Cval sum, S::reg for the dot class's register.  The default, PlusTimes, is the code that
// was there (V(0), av * bv, atomicAdd, unsafeAtomicAdd, +=); plans of mhs_values_plan_create_semiring run the min-plus,
// max-plus and max-min instantiations, at width 1: ds_min_* / ds_max_* in LDS, global_atomic_min_f64 / _max_f64 in
// the global class (FP32 there: a compare-and-swap loop).
// A mixed plan (mhs_values_plan_create_accum: FP32 values, FP64 sums) runs the forward's LDS and dot kernels with an
// accumulator type Acc beside V, the last template parameter (default V: every other plan's kernels are the code that
// was there): value arrays, stages and the B pieces in flight are V; a product is Acc(a) * Acc(b), exact for two floats
// in double; slices, planes and the dot register are Acc, so the LDS add is ds_add_f64; an entry is converted to V
// once, at its store.  Its global class is k_val_global<float>: C's float segment is the accumulator there.
// The mixed instantiations are a translation unit -- a code object -- of their own: mhs_values_mixed.hip includes this
// file with MHS_VALUES_MIXED_TU defined, which leaves the templates, issue_values_mixed and
// init_values_mixed_attributes and takes out everything else; without it this file is every other plan's kernels and
// no mixed one, so its code object holds the kernels it held before there were mixed plans.
#include "mhs_valwalk.hpp"

#include <climits>

namespace mhs {
namespace {

// The columns of the products of row `row` (plan creation: no values), as walk_products of mhs_valwalk.hpp: see(column).
template <int G, class F>
__device__ __forceinline__ void walk_columns(const ValPattern& p, int row, int g, int ng, int t, F see) {
    const int ae = p.Aptr[row + 1];
    for (int k = p.Aptr[row] + g; k < ae; k += ng) {
        const int ac = p.Acol[k];
        const int be = p.Bptr[ac + 1];
        for (int j = p.Bptr[ac] + t; j < be; j += G) see(p.Bcol[j]);
    }
}

#ifndef MHS_VALUES_MIXED_TU  // (plan creation is no part of the mixed plans' translation unit)
// ------------------------------------------------------------- validation ---
// ptr[0] == 0, ptr monotone, ptr[M] == nnz, for A, B and C (which = 0, 1, 2): first bad row per matrix.
__global__ __launch_bounds__(256) void k_val_check_ptr(const int* __restrict__ ptr, int M, int nnz, int* __restrict__ bad) {
    for (int i = blockIdx.x * 256 + threadIdx.x; i < M; i += gridDim.x * 256) {
        const int s = ptr[i], e = ptr[i + 1];
        bool ok = s >= 0 && s <= e && e <= nnz;
        if (i == 0) ok = ok && s == 0;
        if (i == M - 1) ok = ok && e == nnz;
        if (!ok) atomicMin(bad, i);
    }
}
// One wave per row: columns in [0, ncols); strict: ascending without duplicates.
__global__ __launch_bounds__(256) void k_val_check_cols(const int* __restrict__ ptr, const int* __restrict__ col, int M,
                                                        int ncols, int strict, int* __restrict__ bad) {
    const int lane = threadIdx.x & 63;
    for (int i = blockIdx.x * WPB + (threadIdx.x >> 6); i < M; i += gridDim.x * WPB) {
        const int s = ptr[i], e = ptr[i + 1];
        bool ok = true;
        for (int p = s + lane; p < e; p += 64) {
            const int c = col[p];
            ok = ok && c >= 0 && c < ncols;
            if (strict && p > s) ok = ok && col[p - 1] < c;
        }
        if (!ok) atomicMin(bad, i);
    }
}

// --------------------------------------------------------------- classify ---
// One thread per row of C.  FILL false: count the rows and the largest LDS need per class (one
// reservation per block and class; cnt is the counter block of mhs_valplan.hpp).  FILL true: write the rows into
// their class lists, class c's list at the prefix of the counts before it.
// MASKED: the class by val_class_masked -- the row's A entries and, with B^T's row pointer, its dot cost.
// vb: the plan's sum bytes (its width x the bytes of its value type), which the classes and the LDS needs depend on.
template <bool FILL, bool MASKED>
__global__ __launch_bounds__(256) void k_val_classify(ValPattern p, ValMask m, int vb, int* __restrict__ cnt,
                                                      int* __restrict__ lists) {
    __shared__ int s_cnt[VAL_NCLASS], s_need[VAL_NCLASS], s_base[VAL_NCLASS];
    __shared__ unsigned long long s_prod;
    for (int base = blockIdx.x * 256; base < p.M; base += gridDim.x * 256) {
        if (threadIdx.x < VAL_NCLASS) s_cnt[threadIdx.x] = s_need[threadIdx.x] = 0;
        if (threadIdx.x == 0) s_prod = 0;
        __syncthreads();
        const int i = base + threadIdx.x;
        int cls = -1, rank = 0;
        if (i < p.M) {
            const int s = p.Cptr[i], e = p.Cptr[i + 1];
            const int n = e - s;
            long long span = 0, products = 0;
            if (n > 0) span = (long long)p.Ccol[e - 1] - p.Ccol[s] + 1;
            if (n > 0 || MASKED) {  // (a mask's empty rows still have products: mhs_values_info counts them all)
                for (int k = p.Aptr[i]; k < p.Aptr[i + 1]; ++k) {
                    const int ac = p.Acol[k];
                    products += p.Bptr[ac + 1] - p.Bptr[ac];
                }
            }
            if constexpr (MASKED) {
                const int nA = p.Aptr[i + 1] - p.Aptr[i];
                long long steps = 0;
                if (m.tptr && nA > 0 && m.form != VM_PRODUCT)
                    for (int q = s; q < e; ++q) {
                        const int j = p.Ccol[q];
                        steps = val_sat_add(steps, val_dot_steps(m.tptr[j + 1] - m.tptr[j]));
                    }
                cls = val_class_masked(n, span, products, nA, val_sat_mul(nA, steps), m.tptr ? m.form : VM_PRODUCT, m.ratio, vb);
            } else {
                cls = val_class(n, span, products, vb);
            }
            rank = atomicAdd(&s_cnt[cls], 1);
            if (!FILL) {
                atomicMax(&s_need[cls], val_row_need(cls, n, span, vb));
                if (products > 0) atomicAdd(&s_prod, (unsigned long long)products);
            }
        }
        __syncthreads();
        if (!FILL && threadIdx.x == 0 && s_prod > 0)  // the pattern's product count (mhs_values_info)
            atomicAdd((unsigned long long*)(cnt + VAL_CNT_PRODUCTS), s_prod);
        if (threadIdx.x < VAL_NCLASS && s_cnt[threadIdx.x] > 0) {
            const int c = threadIdx.x;
            if (FILL) {
                int off = 0;
                for (int b = 0; b < c; ++b) off += cnt[val_cnt_rows(b)];
                s_base[c] = off + atomicAdd(&cnt[val_cnt_cursor(c)], s_cnt[c]);
            } else {
                atomicAdd(&cnt[val_cnt_rows(c)], s_cnt[c]);
                atomicMax(&cnt[val_cnt_need(c)], s_need[c]);
            }
        }
        __syncthreads();
        if (FILL && cls >= 0) lists[s_base[cls] + rank] = i;
        __syncthreads();
    }
}

// ----------------------------------------------------------------- verify ---
// Pattern-only walk of the shape of the value kernels: one wave per row, every product's column
// must be in the row's C columns.
__global__ __launch_bounds__(256) void k_val_verify(ValPattern p, int* __restrict__ bad) {
    const int lane = threadIdx.x & 63;
    for (int i = blockIdx.x * WPB + (threadIdx.x >> 6); i < p.M; i += gridDim.x * WPB) {
        const int s = p.Cptr[i], n = p.Cptr[i + 1] - s;
        bool ok = true;
        walk_columns<VAL_GROUP>(p, i, lane / VAL_GROUP, 64 / VAL_GROUP, lane % VAL_GROUP,
                                [&](int c) { ok = ok && find_slot(p.Ccol + s, n, c) >= 0; });
        if (!ok) atomicMin(bad, i);
    }
}

// Masked plans, in place of the verify walk: the products whose column is in the row's mask, counted.
__global__ __launch_bounds__(256) void k_val_count_kept(ValPattern p, unsigned long long* __restrict__ kept) {
    __shared__ unsigned long long s_kept;
    if (threadIdx.x == 0) s_kept = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    unsigned long long mine = 0;
    for (int i = blockIdx.x * WPB + (threadIdx.x >> 6); i < p.M; i += gridDim.x * WPB) {
        const int s = p.Cptr[i], n = p.Cptr[i + 1] - s;
        if (n <= 0) continue;
        walk_columns<VAL_GROUP>(p, i, lane / VAL_GROUP, 64 / VAL_GROUP, lane % VAL_GROUP,
                                [&](int c) { mine += find_slot(p.Ccol + s, n, c) >= 0; });
    }
    if (mine) atomicAdd(&s_kept, mine);
    __syncthreads();
    if (threadIdx.x == 0 && s_kept) atomicAdd(kept, s_kept);
}

#endif  // MHS_VALUES_MIXED_TU
// ---------------------------------------------------------- value kernels ---
// Searched sums of one row by `lanes` lanes (lane t): cols / acc are the row's LDS slice, set w's sums the
// plane acc + w * pitch.  walk(pre, add) runs pre() and a sync, then add(column, sums) per product; sync orders
// the steps (a wave's or a block's).  Every set's ds_add has the one slot, so the bank pattern of one set's.
// Acc: the type of the sums (V, or a mixed plan's double); an entry is converted to V at its store.
template <int W, class S = PlusTimes, class V, class Acc, class Sync, class Walk>
__device__ __forceinline__ void row_search(const ValArgs<V>& a, int s, int n, Acc* acc, int* cols, int pitch, int t, int lanes,
                                           Sync sync, Walk walk) {
    const int nw = val_nw<W>(a);
    walk(
        [&] {
            for (int p = t; p < n; p += lanes) {
                cols[p] = a.C.col[s + p];
#pragma unroll
                for (int w = 0; w < W; ++w)
                    if (w < nw) acc[(size_t)w * pitch + p] = S::template identity<Acc>();
            }
        },
        [&](int c, const ValSums<Acc, W>& v) {
            const int slot = find_slot(cols, n, c);
            if (slot >= 0) {
#pragma unroll
                for (int w = 0; w < W; ++w)
                    if (w < nw) S::lds(&acc[(size_t)w * pitch + slot], v.x[w]);  // ds_add_f64 / ds_add_f32, ds_min_* / ds_max_*
            }
        });
    sync();
#pragma unroll
    for (int w = 0; w < W; ++w)
        if (w < nw)
            for (int p = t; p < n; p += lanes) a.C.val[(long long)w * a.sC + (s + p)] = V(acc[(size_t)w * pitch + p]);
    sync();
}
// Span-indexed sums of one row: acc[w * span + col - first], gathered through C.col afterwards.
template <int W, class S = PlusTimes, class V, class Acc, class Sync, class Walk>
__device__ __forceinline__ void row_direct(const ValArgs<V>& a, int s, int n, int first, int span, Acc* acc, int t, int lanes,
                                           Sync sync, Walk walk) {
    const int nw = val_nw<W>(a);
    walk(
        [&] {
#pragma unroll
            for (int w = 0; w < W; ++w)
                if (w < nw)
                    for (int p = t; p < span; p += lanes) acc[(size_t)w * span + p] = S::template identity<Acc>();
        },
        [&](int c, const ValSums<Acc, W>& v) {
            const unsigned slot = (unsigned)(c - first);
            if (slot < (unsigned)span) {
#pragma unroll
                for (int w = 0; w < W; ++w)
                    if (w < nw) S::lds(&acc[(size_t)w * span + slot], v.x[w]);  // ds_add_f64 / ds_add_f32, ds_min_* / ds_max_*
            }
        });
    sync();
    for (int p = t; p < n; p += lanes) {
        const int slot = a.C.col[s + p] - first;
#pragma unroll
        for (int w = 0; w < W; ++w)
            if (w < nw) a.C.val[(long long)w * a.sC + (s + p)] = V(acc[(size_t)w * span + slot]);
    }
    sync();
}

// One row of a wave or block class in the row frame: direct or searched sums over the staged walk.
template <bool DIRECT, int W, class S, class Acc, int CH, class V, class Sync>
__device__ __forceinline__ void row_sums(const ValArgs<V>& a, int row, char* base, int region, int t, int lanes,
                                         ValStage<CH, V, W>& d, Sync sync) {
    val_row<DIRECT, W, Acc>(a, row, base, region, [&](int s, int n, int first, int span, Acc* acc, int* cols) {
        const int pitch = val_slice_entries(region, W * (int)sizeof(Acc));  // (search: the slice's entries, as search_slice)
        auto walk = [&](auto pre, auto add) { walk_staged<VAL_GROUP, W, S, Acc>(a, row, t, lanes, d, sync, pre, add); };
        if constexpr (DIRECT) row_direct<W, S>(a, s, n, first, span, acc, t, lanes, sync, walk);
        else row_search<W, S>(a, s, n, acc, cols, pitch, t, lanes, sync, walk);
    });
}

// Team class: VAL_TEAM_LANES lanes per row, the teams of a wave in step (wave-level ordering).
template <class V, int W, class S = PlusTimes, class Acc = V>
__global__ __launch_bounds__(256) void k_val_team(ValArgs<V> a, const int* __restrict__ list, int count, int region) {
    extern __shared__ __align__(16) char lds[];
    const int team = threadIdx.x / VAL_TEAM_LANES, t = threadIdx.x % VAL_TEAM_LANES;
    const int nw = val_nw<W>(a);
    const ValSlice<Acc> sl = search_slice<Acc, W>(lds + (size_t)team * region, region);
    Acc* acc = sl.val;
    int* cols = sl.cols;
    for (int base = blockIdx.x * VAL_TEAM_ROWS; base < count; base += gridDim.x * VAL_TEAM_ROWS) {
        int s, n;
        const int row = val_team_row(a, list, count, base + team, sl.ne, s, n);
        for (int p = t; p < n; p += VAL_TEAM_LANES) {
            cols[p] = a.C.col[s + p];
#pragma unroll
            for (int w = 0; w < W; ++w)
                if (w < nw) acc[(size_t)w * sl.ne + p] = S::template identity<Acc>();
        }
        vwave_sync();
        if (n > 0)
            walk_products<VAL_TEAM_LANES, W, S, Acc>(a, row, 0, 1, t, [&](int c, const ValSums<Acc, W>& v) {
                const int slot = find_slot(cols, n, c);
                if (slot >= 0) {
#pragma unroll
                    for (int w = 0; w < W; ++w)
                        if (w < nw) S::lds(&acc[(size_t)w * sl.ne + slot], v.x[w]);  // ds_add_f64 / ds_add_f32, ds_min_* / ds_max_*
                }
            });
        vwave_sync();
#pragma unroll
        for (int w = 0; w < W; ++w)
            if (w < nw)
                for (int p = t; p < n; p += VAL_TEAM_LANES) a.C.val[(long long)w * a.sC + (s + p)] = V(acc[(size_t)w * sl.ne + p]);
        vwave_sync();
    }
}

// Wave classes: one wave64 per row, WPB rows per block.
template <class V, int W, bool DIRECT, class S = PlusTimes, class Acc = V>
__global__ __launch_bounds__(256) void k_val_wave(ValArgs<V> a, const int* __restrict__ list, int count, int region) {
    extern __shared__ __align__(16) char lds[];
    __shared__ ValStage<64, V, W> stage[WPB];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    auto sync = [] { vwave_sync(); };
    for (int idx = blockIdx.x * WPB + wave; idx < count; idx += gridDim.x * WPB)
        row_sums<DIRECT, W, S, Acc>(a, list[idx], lds + (size_t)wave * region, region, lane, 64, stage[wave], sync);
}

// Block classes: one block of T threads per row, up to the whole 160 KiB (VAL_BLOCK_BYTES dynamic + the stage).
template <class V, int W, int T, bool DIRECT, class S = PlusTimes, class Acc = V>
__global__ __launch_bounds__(T) void k_val_block(ValArgs<V> a, const int* __restrict__ list, int count, int region) {
    extern __shared__ __align__(16) char lds[];
    __shared__ ValStage<VAL_STAGE, V, W> stage;
    auto sync = [] { __syncthreads(); };
    const XcdStretch x = xcd_stretch(count);
    for (int idx = x.begin; idx < x.end; idx += x.step)
        row_sums<DIRECT, W, S, Acc>(a, list[idx], lds, region, threadIdx.x, T, stage, sync);
}

// Global class: the row's Cval segment -- of every set of the pass -- is the accumulator.
template <class V, int W, class S = PlusTimes>
__global__ __launch_bounds__(1024) void k_val_global(ValArgs<V> a, const int* __restrict__ list, int count) {
    const int t = threadIdx.x;
    const int nw = val_nw<W>(a);
    for (int idx = blockIdx.x; idx < count; idx += gridDim.x) {
        const int row = list[idx];
        const int s = a.C.ptr[row], n = a.C.ptr[row + 1] - s;
#pragma unroll
        for (int w = 0; w < W; ++w)
            if (w < nw)
                for (int p = t; p < n; p += 1024) a.C.val[(long long)w * a.sC + (s + p)] = S::template identity<V>();
        __threadfence();
        __syncthreads();
        walk_products<VAL_GROUP, W, S>(a, row, t / VAL_GROUP, 1024 / VAL_GROUP, t % VAL_GROUP, [&](int c, const ValSums<V, W>& v) {
            const int slot = find_slot(a.C.col + s, n, c);
            if (slot >= 0) {
#pragma unroll
                for (int w = 0; w < W; ++w)  // global_atomic_add_f64 / _f32, global_atomic_min_f64 / _max_f64 (FP32: a loop)
                    if (w < nw) S::glob(&a.C.val[(long long)w * a.sC + (s + slot)], v.x[w]);
            }
        });
    }
}

// Dot class (masked plans): one wave64 per row, WPB rows per block.  Lane l owns the mask entries
// l, l + 64, ... of the row, 64 at a time: for its entry (row, j) it holds B^T row j's bounds, and for
// every A entry of the row -- staged 64 at a time as (column, value) in the wave's static LDS -- finds
// the A column's lower bound in trow[lo0, hi0) and adds av * Bval[tperm[q]] over the equal run (B's
// duplicates, in B's order).  One sum per entry in a register, in A's entry order: no atomics, the
// same bits on every call; the entry is stored once, reached or not.  The register sum is a V.
// W sets: a value per set in the stage, a register sum per set, the one search per (entry, A column);
// each set's sum in the order of the unbatched call, so with its bits.  A mixed plan's register sum is an Acc
// (double) of products formed in it, converted to V at the entry's one store; its stage stays V.
template <class V, int W>
struct DotStage {
    int col[64];
    V av[W][64];
};
template <class V, int W, class S = PlusTimes, class Acc = V>
__global__ __launch_bounds__(256) void k_val_dot(ValArgs<V> a, ValTrans tr, const int* __restrict__ list, int count) {
    __shared__ DotStage<V, W> stage[WPB];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int nw = val_nw<W>(a);
    DotStage<V, W>& d = stage[wave];
    for (int idx = blockIdx.x * WPB + wave; idx < count; idx += gridDim.x * WPB) {
        const int row = list[idx];
        const int s = a.C.ptr[row], n = a.C.ptr[row + 1] - s;
        const int a0 = a.A.ptr[row], ae = a.A.ptr[row + 1];
        for (int p0 = 0; p0 < n; p0 += 64) {
            const int p = p0 + lane;
            int lo0 = 0, hi0 = 0;
            if (p < n) {
                const int j = a.C.col[s + p];
                lo0 = tr.tptr[j];
                hi0 = tr.tptr[j + 1];
            }
            Acc sum[W];
#pragma unroll
            for (int w = 0; w < W; ++w) sum[w] = S::template identity<Acc>();
            for (int k0 = a0; k0 < ae; k0 += 64) {
                const int cnt = ae - k0 < 64 ? ae - k0 : 64;
                if (lane < cnt) {
                    d.col[lane] = a.A.col[k0 + lane];
#pragma unroll
                    for (int w = 0; w < W; ++w)
                        if (w < nw) d.av[w][lane] = a.A.val[(long long)w * a.sA + (k0 + lane)];
                }
                vwave_sync();
                if (lo0 < hi0)
                    for (int e = 0; e < cnt; ++e) {
                        const int ac = d.col[e];
                        int lo = lo0, hi = hi0;
                        while (lo < hi) {
                            const int mid = (lo + hi) >> 1;
                            if (tr.trow[mid] < ac) lo = mid + 1;
                            else hi = mid;
                        }
                        for (; lo < hi0 && tr.trow[lo] == ac; ++lo) {
                            const int q = tr.tperm[lo];
#pragma unroll
                            for (int w = 0; w < W; ++w)
                                if (w < nw) sum[w] = S::reg(sum[w], S::mul(Acc(d.av[w][e]), Acc(a.B.val[(long long)w * a.sB + q])));
                        }
                    }
                vwave_sync();
            }
            if (p < n) {
#pragma unroll
                for (int w = 0; w < W; ++w)
                    if (w < nw) a.C.val[(long long)w * a.sC + (s + p)] = V(sum[w]);
            }
        }
    }
}

// The forward's kernels over the LDS classes' lists (val_lds_kernel), for the value type V and the width W
// and the semiring policy S, with sums of Acc (V; a mixed plan's: double over float)
template <class V, int W, class S = PlusTimes, class Acc = V>
struct ValKernels {
    using Fn = void (*)(ValArgs<V>, const int*, int, int);
    static Fn team() { return k_val_team<V, W, S, Acc>; }
    template <bool DIRECT>
    static Fn wave() { return k_val_wave<V, W, DIRECT, S, Acc>; }
    template <int T, bool DIRECT>
    static Fn block() { return k_val_block<V, W, T, DIRECT, S, Acc>; }
};

// The kernels' static LDS is what the plan header says (val_static_lds: tests/valplan_batched_check.cpp sums it
// with every launch's dynamic bytes)
template <class V, int W>
constexpr bool val_static_lds_holds() {
    return sizeof(ValStage<64, V, W>[WPB]) == val_static_lds(VK_WAVE_DIRECT, sizeof(V), W) &&
           sizeof(ValStage<VAL_STAGE, V, W>) == val_static_lds(VK_BLOCK_SEARCH, sizeof(V), W) &&
           sizeof(DotStage<V, W>[WPB]) == val_static_lds(VK_DOT, sizeof(V), W);
}
static_assert(val_static_lds_holds<double, 1>() && val_static_lds_holds<double, 2>() && val_static_lds_holds<double, 4>() &&
                  val_static_lds_holds<float, 1>() && val_static_lds_holds<float, 2>() && val_static_lds_holds<float, 4>(),
              "val_static_lds is the kernels' static LDS");

// The 1024-thread block kernels of (V, W) for the whole 160 KiB, and the team kernel for its launch cap where
// that is past what a launch may take unasked (val_team_registers: FP64 sums at width 4).  The sum bytes are the
// accumulator's: a mixed plan's stages are float (the static_assert above covers them), its slices double.
template <class V, int W, class S = PlusTimes, class Acc = V>
hipError_t val_register() {
    hipError_t e = val_allow_max_lds<ValKernels<V, W, S, Acc>>();
    constexpr int sb = W * (int)sizeof(Acc);
    if (e == hipSuccess && val_team_registers(sb))
        e = hipFuncSetAttribute((const void*)ValKernels<V, W, S, Acc>::team(), hipFuncAttributeMaxDynamicSharedMemorySize,
                                val_team_launch_cap(sb));
    return e;
}
// One launch over its class's list.  Acc: the LDS and dot kernels' sums; the global class has none but C's segment and
// is k_val_global<V>, which a launch of Acc other than V therefore does not reach (issue_values sends it the native way)
template <class V, int W, class S = PlusTimes, class Acc = V>
void issue_width(const ValLaunch& l, const ValArgs<V>& a, const ValTrans& t, const int* list, hipStream_t s) {
    const dim3 g(l.grid), b(l.block);
    if (const typename ValKernels<V, W, S, Acc>::Fn k = val_lds_kernel<ValKernels<V, W, S, Acc>>(l.kernel, l.block)) {
        hipLaunchKernelGGL(k, g, b, l.lds, s, a, list, l.count, l.region);
    } else if (l.kernel == VK_GLOBAL) {
        if constexpr (sizeof(Acc) == sizeof(V)) hipLaunchKernelGGL((k_val_global<V, W, S>), g, b, 0, s, a, list, l.count);
    } else if (l.kernel == VK_DOT) {
        hipLaunchKernelGGL((k_val_dot<V, W, S, Acc>), g, b, 0, s, a, t, list, l.count);
    }
}

#ifdef MHS_VALUES_MIXED_TU
}  // namespace

// The mixed plans' kernels (FP32 values, FP64 sums), W = 1, 2, 4: their attributes, and one LDS-class or dot launch
hipError_t init_values_mixed_attributes() {
    hipError_t e = val_register<float, 1, PlusTimes, double>();
    if (e == hipSuccess) e = val_register<float, 2, PlusTimes, double>();
    if (e == hipSuccess) e = val_register<float, 4, PlusTimes, double>();
    return e;
}
void issue_values_mixed(const ValLaunch& l, int width, const ValArgs<float>& a, const ValTrans& t, const int* list,
                        hipStream_t s) {
    switch (width) {  // (a width that is none of these made no plan: nothing to launch)
    case 1: return issue_width<float, 1, PlusTimes, double>(l, a, t, list, s);
    case 2: return issue_width<float, 2, PlusTimes, double>(l, a, t, list, s);
    case 4: return issue_width<float, 4, PlusTimes, double>(l, a, t, list, s);
    }
}
#else
// ... of every width on plus-times, and of the three other semirings at their one width
template <class V>
hipError_t val_register_widths() {
    hipError_t e = val_register<V, 1>();
    if (e == hipSuccess) e = val_register<V, 2>();
    if (e == hipSuccess) e = val_register<V, 4>();
    if (e == hipSuccess) e = val_register<V, 1, SrPolicy<SR_MIN_PLUS>>();
    if (e == hipSuccess) e = val_register<V, 1, SrPolicy<SR_MAX_PLUS>>();
    if (e == hipSuccess) e = val_register<V, 1, SrPolicy<SR_MAX_MIN>>();
    return e;
}

int blocks_for(long long items, int per, int cap) {
    long long b = (items + per - 1) / per;
    if (b < 1) b = 1;
    return (int)(b < cap ? b : cap);
}

}  // namespace

hipError_t init_values_attributes() {
    hipError_t e = val_register_widths<double>();
    if (e == hipSuccess) e = val_register_widths<float>();
    if (e == hipSuccess) e = init_values_mixed_attributes();  // the mixed plans' (mhs_values_mixed.hip)
    if (e == hipSuccess) e = init_values_grad_attributes();  // their backward (mhs_values_grad.hip)
    if (e == hipSuccess) e = init_values_subgrad_attributes();  // the semiring plans' subgradient (mhs_values_subgrad.hip)
    if (e == hipSuccess) e = init_values_smooth_attributes();  // the smoothed plans' forward and gradient (mhs_values_smooth.hip)
    return e;
}

void launch_val_check_ptr(const int* ptr, int M, int nnz, int* bad, hipStream_t s) {
    if (M <= 0) return;
    hipLaunchKernelGGL(k_val_check_ptr, dim3(blocks_for(M, 256, 4096)), dim3(256), 0, s, ptr, M, nnz, bad);
}
void launch_val_check_cols(const int* ptr, const int* col, int M, int ncols, bool strict, int* bad, hipStream_t s) {
    if (M <= 0) return;
    hipLaunchKernelGGL(k_val_check_cols, dim3(blocks_for(M, WPB, 16384)), dim3(256), 0, s, ptr, col, M, ncols, strict ? 1 : 0,
                       bad);
}
void launch_val_classify(const ValPattern& p, int vb, int* cnt, int* lists, hipStream_t s) {
    if (p.M <= 0) return;
    const int grid = blocks_for(p.M, 256, 16384);
    hipLaunchKernelGGL((k_val_classify<false, false>), dim3(grid), dim3(256), 0, s, p, ValMask{}, vb, cnt, lists);
    hipLaunchKernelGGL((k_val_classify<true, false>), dim3(grid), dim3(256), 0, s, p, ValMask{}, vb, cnt, lists);
}
void launch_val_classify_masked(const ValPattern& p, const ValMask& m, int vb, int* cnt, int* lists, hipStream_t s) {
    if (p.M <= 0) return;
    const int grid = blocks_for(p.M, 256, 16384);
    hipLaunchKernelGGL((k_val_classify<false, true>), dim3(grid), dim3(256), 0, s, p, m, vb, cnt, lists);
    hipLaunchKernelGGL((k_val_classify<true, true>), dim3(grid), dim3(256), 0, s, p, m, vb, cnt, lists);
}
void launch_val_count_kept(const ValPattern& p, int* cnt, hipStream_t s) {
    if (p.M <= 0) return;
    hipLaunchKernelGGL(k_val_count_kept, dim3(blocks_for(p.M, WPB, 16384)), dim3(256), 0, s, p,
                       (unsigned long long*)(cnt + VAL_CNT_KEPT));
}
void launch_val_verify(const ValPattern& p, int* bad, hipStream_t s) {
    if (p.M <= 0) return;
    hipLaunchKernelGGL(k_val_verify, dim3(blocks_for(p.M, WPB, 16384)), dim3(256), 0, s, p, bad);
}

template <class V>
void issue_values(const ValLaunch& l, int width, int semiring, int accum, const ValArgs<V>& a, const ValTrans& t,
                  const int* list, hipStream_t s) {
    if constexpr (sizeof(V) == VAL_VB_F32) {
        // a mixed plan (plus-times: no other is made): its LDS and dot launches; its global class runs as an FP32 plan's
        if (accum == VAL_ACC_F64 && l.kernel != VK_GLOBAL) {
            if (semiring == SR_PLUS_TIMES) issue_values_mixed(l, width, a, t, list, s);
            return;
        }
    }
    if (semiring != SR_PLUS_TIMES) {  // (width 1: no other plan of such a semiring is made)
        if (width != 1) return;
        switch (semiring) {
        case SR_MIN_PLUS: return issue_width<V, 1, SrPolicy<SR_MIN_PLUS>>(l, a, t, list, s);
        case SR_MAX_PLUS: return issue_width<V, 1, SrPolicy<SR_MAX_PLUS>>(l, a, t, list, s);
        case SR_MAX_MIN: return issue_width<V, 1, SrPolicy<SR_MAX_MIN>>(l, a, t, list, s);
        }
        return;
    }
    switch (width) {  // (a width that is none of these made no plan: nothing to launch)
    case 1: return issue_width<V, 1>(l, a, t, list, s);
    case 2: return issue_width<V, 2>(l, a, t, list, s);
    case 4: return issue_width<V, 4>(l, a, t, list, s);
    }
}
template void issue_values<double>(const ValLaunch&, int, int, int, const ValArgs<double>&, const ValTrans&, const int*,
                                   hipStream_t);
template void issue_values<float>(const ValLaunch&, int, int, int, const ValArgs<float>&, const ValTrans&, const int*, hipStream_t);
#endif  // MHS_VALUES_MIXED_TU

}  // namespace mhs
