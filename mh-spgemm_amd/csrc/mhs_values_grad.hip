// mhs_values_grad.hip -- the backward of the values-only SpGEMM (mhs_spgemm_values_grad): the adjoint of
// (Aval, Bval) -> Cval on a kept plan.
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
#include "mhs_valwalk.hpp"

namespace mhs {
namespace {

// Sum over the G lanes of a group (a power of two); every lane of the group must be here.
template <int G, class V>
__device__ __forceinline__ V group_sum(V v) {
#pragma unroll
    for (int m = G / 2; m > 0; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

// One kept product: B entry q, cotangent gv; sum is the lane's share of the A entry's gradient.
template <class V>
__device__ __forceinline__ void grad_product(const ValGradArgs<V>& a, bool wa, bool wb, int q, V bv, V av, V gv, V& sum) {
    if (wa) sum += bv * gv;
    if (wb) unsafeAtomicAdd(&a.dB[q], av * gv);  // global_atomic_add_f64 / _f32
}

// The staged walk of walk_staged (mhs_values.hip) for a wave's or a block's row, backwards.  The row's
// `lanes` lanes stage up to CH A entries; group g of ng then takes staged entries g, g + ng, ... in
// steps all groups make together, reads its B row VAL_PIECES G-wide pieces at a time, and asks
// look(column, gv) for the cotangent of each product (false: not in the row).  sync() publishes the
// caller's staging of G with the first stage.
template <int G, int CH, class V, class Sync, class Look>
__device__ __forceinline__ void grad_staged(const ValGradArgs<V>& a, int a0, int ae, int t, int lanes, ValStage<CH, V>& d,
                                            Sync sync, Look look) {
    const int g = t / G, ng = lanes / G, tl = t % G;
    const bool wa = a.dA != nullptr, wb = a.dB != nullptr;
    for (int k0 = a0; k0 < ae; k0 += CH) {
        const int cnt = ae - k0 < CH ? ae - k0 : CH;
        if (t < cnt) {
            const int ac = a.A.col[k0 + t];
            const int bs = a.B.ptr[ac];
            d.bs[t] = bs;
            d.len[t] = a.B.ptr[ac + 1] - bs;
            d.av[t] = wb ? a.A.val[k0 + t] : V(0);
        }
        sync();
        for (int e0 = 0; e0 < cnt; e0 += ng) {  // the same trip count in every lane of the row
            const int e = e0 + g;
            const bool on = e < cnt;
            V sum = V(0);
            if (on) {
                const int bs = d.bs[e], len = d.len[e];
                const V av = d.av[e];
                for (int j = tl; j < len; j += VAL_PIECES * G) {
                    int c[VAL_PIECES];
                    V v[VAL_PIECES];
#pragma unroll
                    for (int u = 0; u < VAL_PIECES; ++u) {
                        const int jj = j + u * G;
                        const bool in = jj < len;
                        c[u] = in ? a.B.col[bs + jj] : -1;
                        v[u] = in && wa ? a.B.val[bs + jj] : V(0);
                    }
#pragma unroll
                    for (int u = 0; u < VAL_PIECES; ++u) {
                        V gv;
                        if (c[u] >= 0 && look(c[u], gv)) grad_product(a, wa, wb, bs + j + u * G, v[u], av, gv, sum);
                    }
                }
            }
            // (the group is whole again: its lanes left the B-row loop, and every group makes this step)
            if (wa) {
                sum = group_sum<G>(sum);
                if (on && tl == 0) a.dA[k0 + e] = sum;
            }
        }
        sync();
    }
}

// One row of a wave or block class in the row frame: stage G (and C.col) in the row's LDS slice, then the walk.
template <bool DIRECT, int CH, class V, class Sync>
__device__ __forceinline__ void grad_row(const ValGradArgs<V>& a, int row, char* base, int region, int t, int lanes,
                                         ValStage<CH, V>& d, Sync sync) {
    val_row<DIRECT>(a, row, base, region, [&](int s, int n, int first, int span, V* g, int* cols) {
        const int a0 = a.A.ptr[row], ae = a.A.ptr[row + 1];
        if (a0 >= ae) return;
        if constexpr (DIRECT) {
            for (int p = t; p < span; p += lanes) g[p] = V(0);
            sync();
            for (int p = t; p < n; p += lanes) g[a.C.col[s + p] - first] = a.C.val[s + p];
            grad_staged<VAL_GROUP>(a, a0, ae, t, lanes, d, sync, [&](int c, V& gv) {
                const unsigned slot = (unsigned)(c - first);
                if (slot >= (unsigned)span) return false;
                gv = g[slot];
                return gv != V(0);  // (0: outside the pattern, or a zero cotangent -- nothing to add either way)
            });
        } else {
            for (int p = t; p < n; p += lanes) {
                cols[p] = a.C.col[s + p];
                g[p] = a.C.val[s + p];
            }
            grad_staged<VAL_GROUP>(a, a0, ae, t, lanes, d, sync, [&](int c, V& gv) {
                const int slot = find_slot(cols, n, c);
                if (slot < 0) return false;
                gv = g[slot];
                return true;
            });
        }
    });
}

// Team class: VAL_TEAM_LANES lanes per row, the teams of a wave in step; a team's lanes are the group
// of each of its A entries.
template <class V>
__global__ __launch_bounds__(256) void k_grad_team(ValGradArgs<V> a, const int* __restrict__ list, int count, int region) {
    extern __shared__ __align__(16) char lds[];
    const int team = threadIdx.x / VAL_TEAM_LANES, t = threadIdx.x % VAL_TEAM_LANES;
    const ValSlice<V> sl = search_slice<V>(lds + (size_t)team * region, region);
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
            g[p] = a.C.val[s + p];
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
            V sum = V(0);
            if (on) {
                const int ac = a.A.col[a0 + it];
                const V av = wb ? a.A.val[a0 + it] : V(0);
                const int be = a.B.ptr[ac + 1];
                for (int j = a.B.ptr[ac] + t; j < be; j += VAL_TEAM_LANES) {
                    const int slot = find_slot(cols, n, a.B.col[j]);
                    if (slot >= 0) grad_product(a, wa, wb, j, wa ? a.B.val[j] : V(0), av, g[slot], sum);
                }
            }
            if (wa) {
                sum = group_sum<VAL_TEAM_LANES>(sum);
                if (on && t == 0) a.dA[a0 + it] = sum;
            }
        }
        vwave_sync();
    }
}

// Wave classes: one wave64 per row, WPB rows per block.
template <class V, bool DIRECT>
__global__ __launch_bounds__(256) void k_grad_wave(ValGradArgs<V> a, const int* __restrict__ list, int count, int region) {
    extern __shared__ __align__(16) char lds[];
    __shared__ ValStage<64, V> stage[WPB];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    auto sync = [] { vwave_sync(); };
    for (int idx = blockIdx.x * WPB + wave; idx < count; idx += gridDim.x * WPB)
        grad_row<DIRECT>(a, list[idx], lds + (size_t)wave * region, region, lane, 64, stage[wave], sync);
}

// Block classes: one block of T threads per row, the forward's split of the list over the XCDs.
template <class V, int T, bool DIRECT>
__global__ __launch_bounds__(T) void k_grad_block(ValGradArgs<V> a, const int* __restrict__ list, int count, int region) {
    extern __shared__ __align__(16) char lds[];
    __shared__ ValStage<VAL_STAGE, V> stage;
    auto sync = [] { __syncthreads(); };
    const XcdStretch x = xcd_stretch(count);
    for (int idx = x.begin; idx < x.end; idx += x.step)
        grad_row<DIRECT>(a, list[idx], lds, region, threadIdx.x, T, stage, sync);
}

// Global form: LANES lanes per row (1024: a block per row of the global class; 64: a wave per row, the
// dot rows of a masked plan, which the forward computes per mask entry and the backward walks by
// products -- right for any row, not tuned).  C.col is searched and G read in HBM; nothing is staged.
template <class V, int LANES>
__global__ __launch_bounds__(LANES < 256 ? 256 : LANES) void k_grad_global(ValGradArgs<V> a, const int* __restrict__ list,
                                                                           int count) {
    constexpr int THREADS = LANES < 256 ? 256 : LANES, ROWS = THREADS / LANES, NG = LANES / VAL_GROUP;
    const int t = threadIdx.x % LANES, g = t / VAL_GROUP, tl = t % VAL_GROUP;
    const bool wa = a.dA != nullptr, wb = a.dB != nullptr;
    for (int idx = blockIdx.x * ROWS + threadIdx.x / LANES; idx < count; idx += gridDim.x * ROWS) {
        const int row = list[idx];
        const int s = a.C.ptr[row], n = a.C.ptr[row + 1] - s;
        if (n <= 0) continue;
        const int a0 = a.A.ptr[row], ae = a.A.ptr[row + 1];
        for (int k0 = a0; k0 < ae; k0 += NG) {  // the same trip count in every lane of the row
            const int k = k0 + g;
            const bool on = k < ae;
            V sum = V(0);
            if (on) {
                const int ac = a.A.col[k];
                const V av = wb ? a.A.val[k] : V(0);
                const int be = a.B.ptr[ac + 1];
                for (int j = a.B.ptr[ac] + tl; j < be; j += VAL_GROUP) {
                    const int slot = find_slot(a.C.col + s, n, a.B.col[j]);
                    if (slot >= 0) grad_product(a, wa, wb, j, wa ? a.B.val[j] : V(0), av, a.C.val[s + slot], sum);
                }
            }
            if (wa) {
                sum = group_sum<VAL_GROUP>(sum);
                if (on && tl == 0) a.dA[k] = sum;
            }
        }
    }
}

// The backward's kernels over the LDS classes' lists (val_lds_kernel), for the value type V
template <class V>
struct GradKernels {
    using Fn = void (*)(ValGradArgs<V>, const int*, int, int);
    static Fn team() { return k_grad_team<V>; }
    template <bool DIRECT>
    static Fn wave() { return k_grad_wave<V, DIRECT>; }
    template <int T, bool DIRECT>
    static Fn block() { return k_grad_block<V, T, DIRECT>; }
};

}  // namespace

hipError_t init_values_grad_attributes() {
    const hipError_t e = val_allow_max_lds<GradKernels<double>>();
    return e == hipSuccess ? val_allow_max_lds<GradKernels<float>>() : e;
}

template <class V>
void issue_values_grad(const ValLaunch& l, const ValGradArgs<V>& a, const int* list, hipStream_t s) {
    const dim3 g(l.grid), b(l.block);
    if (const typename GradKernels<V>::Fn k = val_lds_kernel<GradKernels<V>>(l.kernel, l.block)) {
        hipLaunchKernelGGL(k, g, b, l.lds, s, a, list, l.count, l.region);
    } else if (l.kernel == VK_GLOBAL) {  // (plan_grad has no other kernel)
        // 1024 threads a row for the global class, a wave a row for the dot rows
        if (l.block == 1024) hipLaunchKernelGGL((k_grad_global<V, 1024>), g, b, 0, s, a, list, l.count);
        else hipLaunchKernelGGL((k_grad_global<V, 64>), g, b, 0, s, a, list, l.count);
    }
}
template void issue_values_grad<double>(const ValLaunch&, const ValGradArgs<double>&, const int*, hipStream_t);
template void issue_values_grad<float>(const ValLaunch&, const ValGradArgs<float>&, const int*, hipStream_t);

}  // namespace mhs
