// mhs_backwalk.hpp -- the backward walk of a width-1 values plan, once: what the semiring subgradient and witness
// (mhs_values_subgrad.hip) and the smoothed plans' gradient (mhs_values_smooth.hip) run over the plan's backward launch
// list (plan_grad).  It is the walk of the plus-times backward (mhs_values_grad.hip), which keeps its own, written out
// for its widths 1, 2 and 4: its kernels are held to the code they compile to.  Device code only: the two
// files include it, the host side does not.  Everything here sits in an unnamed namespace, as the kernels of those
// files do: each translation unit instantiates the walk for its own rules and shares no kernel with another.
//
// The walk is the forward's with the data flowing the other way: one kernel per product-form class, the row's LDS
// slice holding R::PLANES values per C entry, staged once and read-only after.
//   team, wave-search, block-search   the row's C.col staged as in the forward, the planes beside it
//   wave-direct, block-direct         plane[col - first] over the span, filled with R::fill first
//   global (and a masked plan's dot rows)   C.col searched and the planes' values read in HBM
// All products of one A entry are visited by one lane group and summed in a register per lane; the sum is reduced
// across the group by shuffles and stored once -- no atomics, a fixed order.  The reduction sits in a loop every lane
// of the wave runs the same number of times (a lane without an entry idles through it), after the B-row loop, where
// the group has reconverged.  Both of A's and B's values are read for every product.
//
// A rule R is a type of static __forceinline__ functions; the walk is a template on it.  It supplies
//   Args, V, PLANES         its argument struct (with A, B, C and dA), value type and planes per C entry; the slice
//                           guards are taken at PLANES * sizeof(V)
//   wants(a)                which of dA and dB the launch writes; wa compile-time false: no group sum in the code
//   staged(a, pl, pos)      what plane pl holds of C position pos (the global form reads it from there, in HBM)
//   fill(pl)                what plane pl of a direct span holds outside the pattern
//   pieces<P>(a, f, row, q, k, c, v, av, sum)   one step of the staged walk: the lane's P loaded pieces of A entry
//                           k's B row -- columns c[u] (-1: past the row's end), values v[u], B entries q + u * VAL_GROUP
//                           -- looked up in `row` (BackRow) and summed
//   product(a, f, q, ac, av, src, slot, sum)   one kept product of the team and global forms: B entry q (its value
//                           still to be loaded), A column ac, the planes' values at src.at(pl, slot), the C position
//                           src.s + slot
#pragma once
#include "mhs_valwalk.hpp"

namespace mhs {
namespace {

// The outputs a launch writes: wave-uniform flags (the outputs' pointers)
struct BackWants {
    bool wa, wb;
};

// A staged row, as the walk's rules read it: the planes of its slice and the slot of a column in them (-1: not in
// the row).  s, n: C's segment; direct: columns first .. first + span - 1 and pitch = span; search: the staged columns
// and pitch = the slice's entries.
template <bool DIRECT, class V>
struct BackRow {
    static constexpr bool direct = DIRECT;
    int s, n, first, span, pitch;
    const V* val;
    const int* cols;
    __device__ __forceinline__ int slot(int c) const {
        if constexpr (DIRECT) {
            const unsigned slot = (unsigned)(c - first);
            return slot < (unsigned)span ? (int)slot : -1;
        } else {
            return find_slot(cols, n, c);
        }
    }
    __device__ __forceinline__ V at(int pl, int slot) const { return val[(size_t)pl * pitch + slot]; }
};
// ... and a row of the global form: nothing staged, C.col searched and the planes' values read in HBM
template <class R>
struct BackMem {
    const typename R::Args& a;
    int s, n;
    __device__ __forceinline__ int slot(int c) const { return find_slot(a.C.col + s, n, c); }
    __device__ __forceinline__ typename R::V at(int pl, int slot) const { return R::staged(a, pl, s + slot); }
};

// Sum over the G lanes of a group (a power of two); every lane of the group must be here.
template <int G, class V>
__device__ __forceinline__ V back_group_sum(V v) {
#pragma unroll
    for (int m = G / 2; m > 0; m >>= 1) v += __shfl_xor(v, m);
    return v;
}
// The group's reduction of an A entry's gradient and its one store (position k of A; on: the group has an entry this
// step, tl: the lane within the group).  Every lane of the group must be here.
template <int G, class R>
__device__ __forceinline__ void back_store(const typename R::Args& a, bool on, int tl, int k, typename R::V sum) {
    const typename R::V r = back_group_sum<G>(sum);
    if (on && tl == 0) a.dA[k] = r;
}

// The staged walk of walk_staged (mhs_valwalk.hpp) for a wave's or a block's row, backwards.  The row's `lanes`
// lanes stage up to CH A entries; group g of ng then takes staged entries g, g + ng, ... in steps all groups make
// together, reads its B row VAL_PIECES group-wide pieces at a time, and hands them to the rule.  sync() publishes
// the caller's staging of the planes with the first stage.
template <class R, bool DIRECT, int CH, class Sync>
__device__ __forceinline__ void back_staged(const typename R::Args& a, int a0, int ae, int t, int lanes,
                                            ValStage<CH, typename R::V, 1>& d, Sync sync, const BackRow<DIRECT, typename R::V>& row) {
    using V = typename R::V;
    constexpr int G = VAL_GROUP, P = VAL_PIECES;
    const int g = t / G, ng = lanes / G, tl = t % G;
    const BackWants f = R::wants(a);
    for (int k0 = a0; k0 < ae; k0 += CH) {
        const int cnt = ae - k0 < CH ? ae - k0 : CH;
        if (t < cnt) {
            const int ac = a.A.col[k0 + t];
            const int bs = a.B.ptr[ac];
            d.bs[t] = bs;
            d.len[t] = a.B.ptr[ac + 1] - bs;
            d.av[t] = a.A.val[k0 + t];
        }
        sync();
        for (int e0 = 0; e0 < cnt; e0 += ng) {  // the same trip count in every lane of the row
            const int e = e0 + g;
            const bool on = e < cnt;
            V sum = V(0);
            if (on) {
                const int bs = d.bs[e], len = d.len[e];
                const V av = d.av[e];
                for (int j = tl; j < len; j += P * G) {
                    int c[P];
                    V v[P];
#pragma unroll
                    for (int u = 0; u < P; ++u) {
                        const int jj = j + u * G;
                        const bool in = jj < len;
                        c[u] = in ? a.B.col[bs + jj] : -1;
                        v[u] = in ? a.B.val[bs + jj] : V(0);
                    }
                    R::template pieces<P>(a, f, row, bs + j, k0 + e, c, v, av, sum);
                }
            }
            // (the group is whole again: its lanes left the B-row loop, and every group makes this step)
            if (f.wa) back_store<G, R>(a, on, tl, k0 + e, sum);
        }
        sync();
    }
}

// One row of a wave or block class in the row frame: stage the planes (and C.col) in the row's LDS slice, then the
// walk.  Direct: the span filled with R::fill, then the row's entries scattered by column; a column outside the
// pattern reads the fill.
template <class R, bool DIRECT, int CH, class Sync>
__device__ __forceinline__ void back_row(const typename R::Args& a, int row, char* base, int region, int t, int lanes,
                                         ValStage<CH, typename R::V, 1>& d, Sync sync) {
    using V = typename R::V;
    val_row<DIRECT, R::PLANES>(a, row, base, region, [&](int s, int n, int first, int span, V* val, int* cols) {
        const int a0 = a.A.ptr[row], ae = a.A.ptr[row + 1];
        if (a0 >= ae) return;
        // the pitch of the planes: the span, or the slice's entries (as search_slice)
        const int pitch = DIRECT ? span : val_slice_entries(region, R::PLANES * (int)sizeof(V));
        if constexpr (DIRECT) {
#pragma unroll
            for (int pl = 0; pl < R::PLANES; ++pl)
                for (int p = t; p < span; p += lanes) val[(size_t)pl * span + p] = R::fill(pl);
            sync();
        }
        for (int p = t; p < n; p += lanes) {
            int slot = p;
            if constexpr (DIRECT) slot = a.C.col[s + p] - first;
            else cols[p] = a.C.col[s + p];
#pragma unroll
            for (int pl = 0; pl < R::PLANES; ++pl) val[(size_t)pl * pitch + slot] = R::staged(a, pl, s + p);
        }
        back_staged<R>(a, a0, ae, t, lanes, d, sync, BackRow<DIRECT, V>{s, n, first, span, pitch, val, cols});
    });
}

// One A entry (position k) in the team and global forms: its B row strided over by the G lanes of its group (lane
// tl), each product's column looked up in src and a kept product handed to the rule.
template <int G, class R, class Src>
__device__ __forceinline__ void back_entry(const typename R::Args& a, BackWants f, int k, int tl, const Src& src,
                                           typename R::V& sum) {
    const int ac = a.A.col[k];
    const typename R::V av = a.A.val[k];
    const int be = a.B.ptr[ac + 1];
    for (int j = a.B.ptr[ac] + tl; j < be; j += G) {
        const int slot = src.slot(a.B.col[j]);
        if (slot >= 0) R::product(a, f, j, ac, av, src, slot, sum);
    }
}

// Team class: VAL_TEAM_LANES lanes per row, the teams of a wave in step; a team's lanes are the group
// of each of its A entries.
template <class R>
__global__ __launch_bounds__(256) void k_back_team(typename R::Args a, const int* __restrict__ list, int count, int region) {
    using V = typename R::V;
    extern __shared__ __align__(16) char lds[];
    const int team = threadIdx.x / VAL_TEAM_LANES, t = threadIdx.x % VAL_TEAM_LANES;
    const ValSlice<V> sl = search_slice<V, R::PLANES>(lds + (size_t)team * region, region);
    const BackWants f = R::wants(a);
    for (int base = blockIdx.x * VAL_TEAM_ROWS; base < count; base += gridDim.x * VAL_TEAM_ROWS) {
        int s, n, a0 = 0, nA = 0;
        const int row = val_team_row(a, list, count, base + team, sl.ne, s, n);
        if (n > 0) {
            a0 = a.A.ptr[row];
            nA = a.A.ptr[row + 1] - a0;
        }
        for (int p = t; p < n; p += VAL_TEAM_LANES) {
            sl.cols[p] = a.C.col[s + p];
#pragma unroll
            for (int pl = 0; pl < R::PLANES; ++pl) sl.val[(size_t)pl * sl.ne + p] = R::staged(a, pl, s + p);
        }
        // every lane of the wave makes as many steps as its longest A row has entries
        int steps = nA;
#pragma unroll
        for (int m = VAL_TEAM_LANES; m < 64; m <<= 1) {
            const int o = __shfl_xor(steps, m);
            steps = o > steps ? o : steps;
        }
        steps = __builtin_amdgcn_readfirstlane(steps);
        vwave_sync();
        const BackRow<false, V> src{s, n, 0, 0, sl.ne, sl.val, sl.cols};
        for (int it = 0; it < steps; ++it) {
            const bool on = it < nA;
            V sum = V(0);
            if (on) back_entry<VAL_TEAM_LANES, R>(a, f, a0 + it, t, src, sum);
            if (f.wa) back_store<VAL_TEAM_LANES, R>(a, on, t, a0 + it, sum);
        }
        vwave_sync();
    }
}

// Wave classes: one wave64 per row, WPB rows per block.
template <class R, bool DIRECT>
__global__ __launch_bounds__(256) void k_back_wave(typename R::Args a, const int* __restrict__ list, int count, int region) {
    extern __shared__ __align__(16) char lds[];
    __shared__ ValStage<64, typename R::V, 1> stage[WPB];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    auto sync = [] { vwave_sync(); };
    for (int idx = blockIdx.x * WPB + wave; idx < count; idx += gridDim.x * WPB)
        back_row<R, DIRECT>(a, list[idx], lds + (size_t)wave * region, region, lane, 64, stage[wave], sync);
}

// Block classes: one block of T threads per row, the forward's split of the list over the XCDs.
template <class R, int T, bool DIRECT>
__global__ __launch_bounds__(T) void k_back_block(typename R::Args a, const int* __restrict__ list, int count, int region) {
    extern __shared__ __align__(16) char lds[];
    __shared__ ValStage<VAL_STAGE, typename R::V, 1> stage;
    auto sync = [] { __syncthreads(); };
    const XcdStretch x = xcd_stretch(count);
    for (int idx = x.begin; idx < x.end; idx += x.step)
        back_row<R, DIRECT>(a, list[idx], lds, region, threadIdx.x, T, stage, sync);
}

// Global form: LANES lanes per row (1024: a block per row of the global class; 64: a wave per row, the
// dot rows of a masked plan, which the forward computes per mask entry and the backward walks by
// products -- right for any row, not tuned).  C.col is searched and the planes read in HBM; nothing is staged.
template <class R, int LANES>
__global__ __launch_bounds__(LANES < 256 ? 256 : LANES) void k_back_global(typename R::Args a, const int* __restrict__ list,
                                                                           int count) {
    using V = typename R::V;
    constexpr int THREADS = LANES < 256 ? 256 : LANES, ROWS = THREADS / LANES, NG = LANES / VAL_GROUP;
    const int t = threadIdx.x % LANES, g = t / VAL_GROUP, tl = t % VAL_GROUP;
    const BackWants f = R::wants(a);
    for (int idx = blockIdx.x * ROWS + threadIdx.x / LANES; idx < count; idx += gridDim.x * ROWS) {
        const int row = list[idx];
        const int s = a.C.ptr[row], n = a.C.ptr[row + 1] - s;
        if (n <= 0) continue;
        const int a0 = a.A.ptr[row], ae = a.A.ptr[row + 1];
        const BackMem<R> src{a, s, n};
        for (int k0 = a0; k0 < ae; k0 += NG) {  // the same trip count in every lane of the row
            const int k = k0 + g;
            const bool on = k < ae;
            V sum = V(0);
            if (on) back_entry<VAL_GROUP, R>(a, f, k, tl, src, sum);
            if (f.wa) back_store<VAL_GROUP, R>(a, on, tl, k, sum);
        }
    }
}

// A rule's kernels over the LDS classes' lists (val_lds_kernel)
template <class R>
struct BackKernels {
    using Fn = void (*)(typename R::Args, const int*, int, int);
    static Fn team() { return k_back_team<R>; }
    template <bool DIRECT>
    static Fn wave() { return k_back_wave<R, DIRECT>; }
    template <int T, bool DIRECT>
    static Fn block() { return k_back_block<R, T, DIRECT>; }
};

// The 1024-thread block kernels of a rule for the whole 160 KiB.  At one or two planes of width 1 no team launch is
// past what a launch may take unasked: the team kernel needs no attribute.  The stages are the plus-times backward's at
// width 1: val_static_lds is these kernels' static LDS too, whatever their planes (tests/valplan_smooth_check.cpp sums
// it with every launch's dynamic bytes).
template <class R>
hipError_t back_register() {
    using V = typename R::V;
    static_assert(sizeof(ValStage<64, V, 1>[WPB]) == val_static_lds(VK_WAVE_DIRECT, sizeof(V), 1) &&
                      sizeof(ValStage<VAL_STAGE, V, 1>) == val_static_lds(VK_BLOCK_SEARCH, sizeof(V), 1),
                  "val_static_lds is the backward kernels' static LDS");
    static_assert(!val_team_registers(R::PLANES * (int)sizeof(V)), "the team kernels need no attribute");
    return val_allow_max_lds<BackKernels<R>>();
}

// One launch of the backward list (plan_grad) over its class's row list
template <class R>
void back_issue(const ValLaunch& l, const typename R::Args& a, const int* list, hipStream_t s) {
    const dim3 g(l.grid), b(l.block);
    if (const typename BackKernels<R>::Fn k = val_lds_kernel<BackKernels<R>>(l.kernel, l.block)) {
        hipLaunchKernelGGL(k, g, b, l.lds, s, a, list, l.count, l.region);
    } else if (l.kernel == VK_GLOBAL) {  // (plan_grad has no other kernel)
        // 1024 threads a row for the global class, a wave a row for the dot rows
        if (l.block == 1024) hipLaunchKernelGGL((k_back_global<R, 1024>), g, b, 0, s, a, list, l.count);
        else hipLaunchKernelGGL((k_back_global<R, 64>), g, b, 0, s, a, list, l.count);
    }
}

}  // namespace
}  // namespace mhs
