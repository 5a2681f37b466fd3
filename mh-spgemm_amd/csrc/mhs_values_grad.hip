// mhs_values_grad.hip -- the backward of the values-only SpGEMM (mhs_spgemm_values_grad and
// mhs_spgemm_values_grad_batched): the adjoint of (Aval, Bval) -> Cval on a kept plan.
//
// With G the cotangent on C's pattern, every product (i, k, j) of the forward -- A entry p = (i, k),
// B entry q = (k, j), slot s of column j in C's row i -- gives
//     dA[p] += Bval[q] * G[s]        dB[q] += Aval[p] * G[s]
// so the backward is the forward's walk with the data flowing the other way: one kernel per product-form
// class on the plan's class lists, with the LDS the class needs for its sums holding the row of G.
//   team, wave-search, block-search   the row's C.col staged as in the forward, its G segment beside it
//   wave-direct, block-direct         g[col - first] over the zeroed span: a column outside the pattern reads 0
//   global (and a masked plan's dot rows)   C.col searched and G read in HBM
// After staging, LDS is read-only.  dA: all products of one A entry are visited by one lane group, summed
// in a register per lane, reduced across the group by shuffles and stored once -- no atomics, a fixed
// order.  The reduction sits in a loop every lane of the wave runs the same number of times (a lane
// without an entry idles through it), after the B-row loop, where the group has reconverged.
// dB: one global_atomic_add_f64 (FP32 plans: global_atomic_add_f32) per kept product into the zero-filled
// dB; a group's lanes hit consecutive entries of one B row.  Every kernel is a template on the plan's value
// type V: G in LDS, the register sums of dA and the atomics are all V.  Which sides are wanted is a wave-uniform flag (the output's pointer):
// a dA-only call issues no atomic and reads no Aval, a dB-only call reads no Bval.
// Every kernel is also a template on the plan's width W (1, 2 or 4; W = 1 is the unbatched kernel): a pass of a
// batched call walks the pattern once for its nw <= W sets (ValGradArgs).  The row's LDS slice holds W cotangent
// planes, set-major as the forward's sums -- g[w * pitch + slot], the one column array behind them -- and per
// product the B column, the slot and the staged bounds are found once, then W value loads, W register sums and W
// atomics follow; a set w >= nw is neither loaded nor summed nor stored.  A lane's products of one A entry come
// in ascending j whatever the piece count and every class reduces over the same lanes at every width, so a set's
// dA has the bits of the unbatched call on its values.
#include "mhs_valwalk.hpp"

namespace mhs {
namespace {

// The sets of the pass: W = 1 reads no field of the batch
template <int W, class V>
__device__ __forceinline__ int grad_nw(const ValGradArgs<V>& a) {
    return W == 1 ? 1 : a.nw;
}

// Sum over the G lanes of a group (a power of two); every lane of the group must be here.
template <int G, class V>
__device__ __forceinline__ V group_sum(V v) {
#pragma unroll
    for (int m = G / 2; m > 0; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

// One kept product: B entry q, and per set w < nw its B value, A value and cotangent; sum[w] is the lane's
// share of the A entry's gradient in set w.
template <int W, class V>
__device__ __forceinline__ void grad_product(const ValGradArgs<V>& a, bool wa, bool wb, int nw, int q, const V (&bv)[W],
                                             const V (&av)[W], const V (&gv)[W], V (&sum)[W]) {
#pragma unroll
    for (int w = 0; w < W; ++w)
        if (w < nw) {
            if (wa) sum[w] += bv[w] * gv[w];
            if (wb) unsafeAtomicAdd(&a.dB[(long long)w * a.sDB + q], av[w] * gv[w]);  // global_atomic_add_f64 / _f32
        }
}

// The group's reduction of an A entry's gradient and its one store per set (position k of A; on: the group has
// an entry this step, tl: the lane within the group).  Every lane of the group must be here.
template <int G, int W, class V>
__device__ __forceinline__ void grad_store(const ValGradArgs<V>& a, int nw, bool on, int tl, int k, V (&sum)[W]) {
#pragma unroll
    for (int w = 0; w < W; ++w)
        if (w < nw) {
            const V r = group_sum<G>(sum[w]);
            if (on && tl == 0) a.dA[(long long)w * a.sDA + k] = r;
        }
}

// The staged walk of walk_staged (mhs_valwalk.hpp) for a wave's or a block's row, backwards.  The row's
// `lanes` lanes stage up to CH A entries; group g of ng then takes staged entries g, g + ng, ... in
// steps all groups make together, reads its B row val_pieces(W) G-wide pieces at a time, and asks
// look(column, gv) for the cotangents of each product (false: not in the row).  sync() publishes the
// caller's staging of G with the first stage.  W > 1: the stage holds (start, length) only, and a group reads
// each set's A value at the entry's A position.
template <int G, int W, int CH, class V, class Sync, class Look>
__device__ __forceinline__ void grad_staged(const ValGradArgs<V>& a, int a0, int ae, int t, int lanes, ValStage<CH, V, W>& d,
                                            Sync sync, Look look) {
    constexpr int P = val_pieces(W);
    const int nw = grad_nw<W>(a);
    const int g = t / G, ng = lanes / G, tl = t % G;
    const bool wa = a.dA != nullptr, wb = a.dB != nullptr;
    for (int k0 = a0; k0 < ae; k0 += CH) {
        const int cnt = ae - k0 < CH ? ae - k0 : CH;
        if (t < cnt) {
            const int ac = a.A.col[k0 + t];
            const int bs = a.B.ptr[ac];
            d.bs[t] = bs;
            d.len[t] = a.B.ptr[ac + 1] - bs;
            if constexpr (W == 1) d.av[t] = wb ? a.A.val[k0 + t] : V(0);
        }
        sync();
        for (int e0 = 0; e0 < cnt; e0 += ng) {  // the same trip count in every lane of the row
            const int e = e0 + g;
            const bool on = e < cnt;
            V sum[W];
#pragma unroll
            for (int w = 0; w < W; ++w) sum[w] = V(0);
            if (on) {
                const int bs = d.bs[e], len = d.len[e];
                V av[W];
                if constexpr (W == 1) {
                    av[0] = d.av[e];
                } else {
#pragma unroll
                    for (int w = 0; w < W; ++w)
                        if (w < nw) av[w] = wb ? a.A.val[(long long)w * a.sA + (k0 + e)] : V(0);
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
                            if (w < nw) v[u][w] = in && wa ? a.B.val[(long long)w * a.sB + (bs + jj)] : V(0);
                    }
#pragma unroll
                    for (int u = 0; u < P; ++u) {
                        V gv[W];
                        if (c[u] >= 0 && look(c[u], gv)) grad_product<W>(a, wa, wb, nw, bs + j + u * G, v[u], av, gv, sum);
                    }
                }
            }
            // (the group is whole again: its lanes left the B-row loop, and every group makes this step)
            if (wa) grad_store<G, W>(a, nw, on, tl, k0 + e, sum);
        }
        sync();
    }
}

// One row of a wave or block class in the row frame: stage G (and C.col) in the row's LDS slice, then the walk.
template <bool DIRECT, int W, int CH, class V, class Sync>
__device__ __forceinline__ void grad_row(const ValGradArgs<V>& a, int row, char* base, int region, int t, int lanes,
                                         ValStage<CH, V, W>& d, Sync sync) {
    val_row<DIRECT, W>(a, row, base, region, [&](int s, int n, int first, int span, V* g, int* cols) {
        const int a0 = a.A.ptr[row], ae = a.A.ptr[row + 1];
        if (a0 >= ae) return;
        const int nw = grad_nw<W>(a);
        if constexpr (DIRECT) {
#pragma unroll
            for (int w = 0; w < W; ++w)
                if (w < nw)
                    for (int p = t; p < span; p += lanes) g[(size_t)w * span + p] = V(0);
            sync();
            for (int p = t; p < n; p += lanes) {
                const int slot = a.C.col[s + p] - first;
#pragma unroll
                for (int w = 0; w < W; ++w)
                    if (w < nw) g[(size_t)w * span + slot] = a.C.val[(long long)w * a.sG + (s + p)];
            }
            grad_staged<VAL_GROUP, W>(a, a0, ae, t, lanes, d, sync, [&](int c, V(&gv)[W]) {
                const unsigned slot = (unsigned)(c - first);
                if (slot >= (unsigned)span) return false;
                // (0 in every set: outside the pattern, or zero cotangents -- nothing to add either way; a set whose
                // cotangent alone is 0 adds a zero, which changes no sum)
                bool any = false;
#pragma unroll
                for (int w = 0; w < W; ++w)
                    if (w < nw) {
                        gv[w] = g[(size_t)w * span + slot];
                        any = any || gv[w] != V(0);
                    }
                return any;
            });
        } else {
            const int pitch = val_slice_entries(region, W * (int)sizeof(V));  // (the slice's entries, as search_slice)
            for (int p = t; p < n; p += lanes) {
                cols[p] = a.C.col[s + p];
#pragma unroll
                for (int w = 0; w < W; ++w)
                    if (w < nw) g[(size_t)w * pitch + p] = a.C.val[(long long)w * a.sG + (s + p)];
            }
            grad_staged<VAL_GROUP, W>(a, a0, ae, t, lanes, d, sync, [&](int c, V(&gv)[W]) {
                const int slot = find_slot(cols, n, c);
                if (slot < 0) return false;
#pragma unroll
                for (int w = 0; w < W; ++w)
                    if (w < nw) gv[w] = g[(size_t)w * pitch + slot];
                return true;
            });
        }
    });
}

// Team class: VAL_TEAM_LANES lanes per row, the teams of a wave in step; a team's lanes are the group
// of each of its A entries.
template <class V, int W>
__global__ __launch_bounds__(256) void k_grad_team(ValGradArgs<V> a, const int* __restrict__ list, int count, int region) {
    extern __shared__ __align__(16) char lds[];
    const int team = threadIdx.x / VAL_TEAM_LANES, t = threadIdx.x % VAL_TEAM_LANES;
    const int nw = grad_nw<W>(a);
    const ValSlice<V> sl = search_slice<V, W>(lds + (size_t)team * region, region);
    V* g = sl.val;
    int* cols = sl.cols;
    const bool wa = a.dA != nullptr, wb = a.dB != nullptr;
    for (int base = blockIdx.x * VAL_TEAM_ROWS; base < count; base += gridDim.x * VAL_TEAM_ROWS) {
        int s, n, a0 = 0, nA = 0;
        const int row = val_team_row(a, list, count, base + team, sl.ne, s, n);
        if (n > 0) {
            a0 = a.A.ptr[row];
            nA = a.A.ptr[row + 1] - a0;
        }
        for (int p = t; p < n; p += VAL_TEAM_LANES) {
            cols[p] = a.C.col[s + p];
#pragma unroll
            for (int w = 0; w < W; ++w)
                if (w < nw) g[(size_t)w * sl.ne + p] = a.C.val[(long long)w * a.sG + (s + p)];
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
        for (int it = 0; it < steps; ++it) {
            const bool on = it < nA;
            V sum[W];
#pragma unroll
            for (int w = 0; w < W; ++w) sum[w] = V(0);
            if (on) {
                const int ac = a.A.col[a0 + it];
                V av[W];
#pragma unroll
                for (int w = 0; w < W; ++w)
                    if (w < nw) av[w] = wb ? a.A.val[(long long)w * a.sA + (a0 + it)] : V(0);
                const int be = a.B.ptr[ac + 1];
                for (int j = a.B.ptr[ac] + t; j < be; j += VAL_TEAM_LANES) {
                    const int slot = find_slot(cols, n, a.B.col[j]);
                    if (slot >= 0) {
                        V bv[W], gv[W];
#pragma unroll
                        for (int w = 0; w < W; ++w)
                            if (w < nw) {
                                bv[w] = wa ? a.B.val[(long long)w * a.sB + j] : V(0);
                                gv[w] = g[(size_t)w * sl.ne + slot];
                            }
                        grad_product<W>(a, wa, wb, nw, j, bv, av, gv, sum);
                    }
                }
            }
            if (wa) grad_store<VAL_TEAM_LANES, W>(a, nw, on, t, a0 + it, sum);
        }
        vwave_sync();
    }
}

// Wave classes: one wave64 per row, WPB rows per block.
template <class V, int W, bool DIRECT>
__global__ __launch_bounds__(256) void k_grad_wave(ValGradArgs<V> a, const int* __restrict__ list, int count, int region) {
    extern __shared__ __align__(16) char lds[];
    __shared__ ValStage<64, V, W> stage[WPB];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    auto sync = [] { vwave_sync(); };
    for (int idx = blockIdx.x * WPB + wave; idx < count; idx += gridDim.x * WPB)
        grad_row<DIRECT, W>(a, list[idx], lds + (size_t)wave * region, region, lane, 64, stage[wave], sync);
}

// Block classes: one block of T threads per row, the forward's split of the list over the XCDs.
template <class V, int W, int T, bool DIRECT>
__global__ __launch_bounds__(T) void k_grad_block(ValGradArgs<V> a, const int* __restrict__ list, int count, int region) {
    extern __shared__ __align__(16) char lds[];
    __shared__ ValStage<VAL_STAGE, V, W> stage;
    auto sync = [] { __syncthreads(); };
    const XcdStretch x = xcd_stretch(count);
    for (int idx = x.begin; idx < x.end; idx += x.step)
        grad_row<DIRECT, W>(a, list[idx], lds, region, threadIdx.x, T, stage, sync);
}

// Global form: LANES lanes per row (1024: a block per row of the global class; 64: a wave per row, the
// dot rows of a masked plan, which the forward computes per mask entry and the backward walks by
// products -- right for any row, not tuned).  C.col is searched and G read in HBM; nothing is staged.
template <class V, int W, int LANES>
__global__ __launch_bounds__(LANES < 256 ? 256 : LANES) void k_grad_global(ValGradArgs<V> a, const int* __restrict__ list,
                                                                           int count) {
    constexpr int THREADS = LANES < 256 ? 256 : LANES, ROWS = THREADS / LANES, NG = LANES / VAL_GROUP;
    const int t = threadIdx.x % LANES, g = t / VAL_GROUP, tl = t % VAL_GROUP;
    const int nw = grad_nw<W>(a);
    const bool wa = a.dA != nullptr, wb = a.dB != nullptr;
    for (int idx = blockIdx.x * ROWS + threadIdx.x / LANES; idx < count; idx += gridDim.x * ROWS) {
        const int row = list[idx];
        const int s = a.C.ptr[row], n = a.C.ptr[row + 1] - s;
        if (n <= 0) continue;
        const int a0 = a.A.ptr[row], ae = a.A.ptr[row + 1];
        for (int k0 = a0; k0 < ae; k0 += NG) {  // the same trip count in every lane of the row
            const int k = k0 + g;
            const bool on = k < ae;
            V sum[W];
#pragma unroll
            for (int w = 0; w < W; ++w) sum[w] = V(0);
            if (on) {
                const int ac = a.A.col[k];
                V av[W];
#pragma unroll
                for (int w = 0; w < W; ++w)
                    if (w < nw) av[w] = wb ? a.A.val[(long long)w * a.sA + k] : V(0);
                const int be = a.B.ptr[ac + 1];
                for (int j = a.B.ptr[ac] + tl; j < be; j += VAL_GROUP) {
                    const int slot = find_slot(a.C.col + s, n, a.B.col[j]);
                    if (slot >= 0) {
                        V bv[W], gv[W];
#pragma unroll
                        for (int w = 0; w < W; ++w)
                            if (w < nw) {
                                bv[w] = wa ? a.B.val[(long long)w * a.sB + j] : V(0);
                                gv[w] = a.C.val[(long long)w * a.sG + (s + slot)];
                            }
                        grad_product<W>(a, wa, wb, nw, j, bv, av, gv, sum);
                    }
                }
            }
            if (wa) grad_store<VAL_GROUP, W>(a, nw, on, tl, k, sum);
        }
    }
}

// The backward's kernels over the LDS classes' lists (val_lds_kernel), for the value type V and the width W
template <class V, int W>
struct GradKernels {
    using Fn = void (*)(ValGradArgs<V>, const int*, int, int);
    static Fn team() { return k_grad_team<V, W>; }
    template <bool DIRECT>
    static Fn wave() { return k_grad_wave<V, W, DIRECT>; }
    template <int T, bool DIRECT>
    static Fn block() { return k_grad_block<V, W, T, DIRECT>; }
};

// The backward's stages are the forward's: val_static_lds is its kernels' static LDS too
// (tests/gradplan_batched_check.cpp sums it with every launch's dynamic bytes)
template <class V, int W>
constexpr bool grad_static_lds_holds() {
    return sizeof(ValStage<64, V, W>[WPB]) == val_static_lds(VK_WAVE_DIRECT, sizeof(V), W) &&
           sizeof(ValStage<VAL_STAGE, V, W>) == val_static_lds(VK_BLOCK_SEARCH, sizeof(V), W);
}
static_assert(grad_static_lds_holds<double, 1>() && grad_static_lds_holds<double, 2>() && grad_static_lds_holds<double, 4>() &&
                  grad_static_lds_holds<float, 1>() && grad_static_lds_holds<float, 2>() && grad_static_lds_holds<float, 4>(),
              "val_static_lds is the backward kernels' static LDS");

// The 1024-thread block kernels of (V, W) for the whole 160 KiB, and the team kernel for its launch cap where
// that is past what a launch may take unasked (val_team_registers: FP64 at width 4), as the forward registers its own
template <class V, int W>
hipError_t grad_register() {
    hipError_t e = val_allow_max_lds<GradKernels<V, W>>();
    constexpr int sb = W * (int)sizeof(V);
    if (e == hipSuccess && val_team_registers(sb))
        e = hipFuncSetAttribute((const void*)GradKernels<V, W>::team(), hipFuncAttributeMaxDynamicSharedMemorySize,
                                val_team_launch_cap(sb));
    return e;
}
template <class V>
hipError_t grad_register_widths() {
    hipError_t e = grad_register<V, 1>();
    if (e == hipSuccess) e = grad_register<V, 2>();
    if (e == hipSuccess) e = grad_register<V, 4>();
    return e;
}

template <class V, int W>
void issue_grad_width(const ValLaunch& l, const ValGradArgs<V>& a, const int* list, hipStream_t s) {
    const dim3 g(l.grid), b(l.block);
    if (const typename GradKernels<V, W>::Fn k = val_lds_kernel<GradKernels<V, W>>(l.kernel, l.block)) {
        hipLaunchKernelGGL(k, g, b, l.lds, s, a, list, l.count, l.region);
    } else if (l.kernel == VK_GLOBAL) {  // (plan_grad has no other kernel)
        // 1024 threads a row for the global class, a wave a row for the dot rows
        if (l.block == 1024) hipLaunchKernelGGL((k_grad_global<V, W, 1024>), g, b, 0, s, a, list, l.count);
        else hipLaunchKernelGGL((k_grad_global<V, W, 64>), g, b, 0, s, a, list, l.count);
    }
}

}  // namespace

hipError_t init_values_grad_attributes() {
    hipError_t e = grad_register_widths<double>();
    if (e == hipSuccess) e = grad_register_widths<float>();
    // A mixed plan (FP32 values, FP64 sums) runs the float kernels on a launch list planned at sb = 8 W: at W = 4 its
    // team launch is the FP64 one, past what the float team kernel's own sb = 16 asks for
    static_assert(!val_team_registers(val_sum_bytes(VAL_VB_F32, 2, VAL_ACC_F64)) &&
                      val_team_registers(val_sum_bytes(VAL_VB_F32, 4, VAL_ACC_F64)),
                  "of the mixed plans, width 4 alone has a team launch to register");
    if (e == hipSuccess)
        e = hipFuncSetAttribute((const void*)GradKernels<float, 4>::team(), hipFuncAttributeMaxDynamicSharedMemorySize,
                                val_team_launch_cap(val_sum_bytes(VAL_VB_F32, 4, VAL_ACC_F64)));
    return e;
}

template <class V>
void issue_values_grad(const ValLaunch& l, int width, const ValGradArgs<V>& a, const int* list, hipStream_t s) {
    switch (width) {  // (a width that is none of these made no plan: nothing to launch)
    case 1: return issue_grad_width<V, 1>(l, a, list, s);
    case 2: return issue_grad_width<V, 2>(l, a, list, s);
    case 4: return issue_grad_width<V, 4>(l, a, list, s);
    }
}
template void issue_values_grad<double>(const ValLaunch&, int, const ValGradArgs<double>&, const int*, hipStream_t);
template void issue_values_grad<float>(const ValLaunch&, int, const ValGradArgs<float>&, const int*, hipStream_t);

}  // namespace mhs
