// mhs_values_subgrad.hip -- the subgradient of a semiring values plan (mhs_spgemm_values_subgrad): the backward of
// (Aval, Bval) -> Cval under min-plus, max-plus and max-min on a kept plan, at width 1.
//
// The rule (include/mhspgemm.h): a kept product (A entry p, B entry q, C slot s) is a winner of s when
// mul(Aval[p], Bval[q]) == Cval[s] and Cval[s] is not the identity of add (SrValue<SR>::wins); ties[s] counts the
// winners of s; each carries w = G[s] / ties[s], handed to dA[p] and dB[q] by the gradient of mul (share_a, share_b).
// The forward is bit-identical to a sequential evaluation and mul is formed here with the same one rounding, so the
// comparison is an equality of values, and every reached entry that is neither NaN nor the identity has a winner.
//
// It is the plus-times backward's walk (mhs_values_grad.hip) over the same launch list, twice: the row frame, the
// stage of A entries, the lane groups, the slice guards and the static LDS are those of k_grad_*.  The LDS plane that
// holds the cotangent there holds Cval here, staged the same way -- the winner test is what every product needs, the
// cotangent only what a winner needs, and winners number about nnz(C):
//   team, wave-search, block-search   the row's C.col staged, its Cval segment beside it; a winner's position is s + slot
//   wave-direct, block-direct         c[col - first] over the span filled with NaN: a column outside the pattern
//                                     compares equal to nothing; a winner finds its position by find_slot in C.col + s
//                                     in memory, inside the few positions its place in the span leaves open
//   global (and a masked plan's dot rows)   C.col searched and Cval read in HBM
// Pass 1: every winner adds 1 to ties[position] (an integer global atomic without return).  Pass 2: every winner loads
// G and ties at its position, forms w, feeds the register sum of its A entry -- reduced across the lane group by
// shuffles and stored once, in a fixed order, as grad_store does -- and adds its share to dB[q] by one unsafeAtomicAdd.
// In the wave and block walks a lane tests its VAL_PIECES pieces on LDS first and then takes its winners one after another.
// After staging LDS is read-only.  Which sides are wanted is a wave-uniform flag (the output's pointer).
//
// Pass 3 is the witness (mhs_spgemm_values_witness): the same walks and the same winner test once more, on their own
// call.  wit is filled with 0xFF bytes by the caller -- -1 as an int, the largest unsigned -- and every winner takes the
// unsigned minimum of its inner index k = A.col of its A entry into wit[position] (an integer global atomic without
// return): the smallest k among the winners, -1 where there is none, whatever the order.  It forms no weight, reduces
// nothing over the group and stores no gradient; the staged walk, whose stage keeps no column, reloads A.col for a
// winner (one address over the group).
#include "mhs_valwalk.hpp"

namespace mhs {
namespace {

// Sum over the G lanes of a group (a power of two); every lane of the group must be here.
template <int G, class V>
__device__ __forceinline__ V sub_group_sum(V v) {
#pragma unroll
    for (int m = G / 2; m > 0; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

// One winner: B entry q, C position pos, its operands; sum is the lane's share of the A entry's gradient; k the inner
// index of the product, the column of its A entry (read by pass 3 only).
template <class S, int PASS, class V>
__device__ __forceinline__ void sub_winner(const ValSubArgs<V>& a, bool wa, bool wb, int q, int pos, V av, V bv, V& sum, int k) {
    if constexpr (PASS == 1) {
        (void)__hip_atomic_fetch_add(a.ties + pos, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // global_atomic_add_u32
    } else if constexpr (PASS == 3) {
        // wit is -1 = 0xFFFFFFFF until a winner comes: the unsigned minimum is the smallest k (k >= 0)
        // (a plain load of wit[pos] first, to skip the atomic where it is already <= k, was measured and lost: DESIGN 18)
        (void)__hip_atomic_fetch_min((unsigned*)a.wit + pos, (unsigned)k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // global_atomic_umin
    } else {
        const V w = a.G[pos] / V(a.ties[pos]);  // (ties >= 1: pass 1 counted this winner)
        if (wa) sum += S::share_a(av, bv, w);
        if (wb) {
            const V sb = S::share_b(av, bv, w);
            if (sb != V(0)) unsafeAtomicAdd(a.dB + q, sb);  // global_atomic_add_f64 / _f32 (a NaN share is added)
        }
    }
}

// The group's reduction of an A entry's gradient and its one store (pass 2, dA wanted); every lane of the group
// must be here.
template <int G, class V>
__device__ __forceinline__ void sub_store(const ValSubArgs<V>& a, bool on, int tl, int k, V sum) {
    const V r = sub_group_sum<G>(sum);
    if (on && tl == 0) a.dA[k] = r;
}

// grad_staged's walk at width 1.  look(column, cv) gives the handle of the column in the row's staged plane and its
// Cval (-1: not in the row); where(handle, column) the C position of a winner (-1: none).
template <int G, class S, int PASS, int CH, class V, class Sync, class Look, class Where>
__device__ __forceinline__ void sub_staged(const ValSubArgs<V>& a, int a0, int ae, int t, int lanes, ValStage<CH, V, 1>& d,
                                           Sync sync, Look look, Where where) {
    constexpr int P = VAL_PIECES;
    const int g = t / G, ng = lanes / G, tl = t % G;
    const bool wa = PASS == 2 && a.dA != nullptr, wb = PASS == 2 && a.dB != nullptr;
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
                    // the winner test of the P pieces on LDS alone, then the lane's winners in ascending u: the wave
                    // makes as many trips as its lane with the most winners, not P -- what a winner costs (its position,
                    // the atomic, G and ties) is then paid about per winner, not per piece
                    int h[P];
                    unsigned left = 0;
#pragma unroll
                    for (int u = 0; u < P; ++u) {
                        V cv;
                        h[u] = c[u] >= 0 ? look(c[u], cv) : -1;
                        if (h[u] >= 0 && S::wins(av, v[u], cv)) left |= 1u << u;
                    }
                    while (left) {
                        const int u = __builtin_ctz(left);
                        left &= left - 1;
                        int hu = h[0], cu = c[0];
                        V vu = v[0];
#pragma unroll
                        for (int w = 1; w < P; ++w)
                            if (u == w) hu = h[w], cu = c[w], vu = v[w];
                        const int pos = where(hu, cu);
                        // (the stage keeps no column: pass 3 reloads its A entry's, one address over the group)
                        if (pos >= 0) sub_winner<S, PASS>(a, wa, wb, bs + j + u * G, pos, av, vu, sum, PASS == 3 ? a.A.col[k0 + e] : 0);
                    }
                }
            }
            // (the group is whole again: its lanes left the B-row loop, and every group makes this step)
            if (wa) sub_store<G>(a, on, tl, k0 + e, sum);
        }
        sync();
    }
}

// One row of a wave or block class in the row frame: stage Cval (and C.col) in the row's LDS slice, then the walk.
template <bool DIRECT, class S, int PASS, int CH, class V, class Sync>
__device__ __forceinline__ void sub_row(const ValSubArgs<V>& a, int row, char* base, int region, int t, int lanes,
                                        ValStage<CH, V, 1>& d, Sync sync) {
    val_row<DIRECT, 1>(a, row, base, region, [&](int s, int n, int first, int span, V* cv, int* cols) {
        const int a0 = a.A.ptr[row], ae = a.A.ptr[row + 1];
        if (a0 >= ae) return;
        if constexpr (DIRECT) {
            const V nan = std::numeric_limits<V>::quiet_NaN();
            for (int p = t; p < span; p += lanes) cv[p] = nan;
            sync();
            for (int p = t; p < n; p += lanes) cv[a.C.col[s + p] - first] = a.C.val[s + p];
            sub_staged<VAL_GROUP, S, PASS>(
                a, a0, ae, t, lanes, d, sync,
                [&](int c, V& x) {
                    const unsigned slot = (unsigned)(c - first);
                    if (slot >= (unsigned)span) return -1;
                    x = cv[slot];  // (NaN outside the pattern: no winner)
                    return (int)slot;
                },
                [&](int slot, int c) {
                    // C's columns ascend strictly: at most `slot` of them lie before column first + slot and at most
                    // span - 1 - slot behind it, so its position is in [slot - (span - n), slot] -- on a dense row a
                    // step or two of find_slot in C.col + s instead of log2(n)
                    const int lo = slot - (span - n) > 0 ? slot - (span - n) : 0;
                    const int hi = slot + 1 < n ? slot + 1 : n;
                    const int at = find_slot(a.C.col + s + lo, hi - lo, c);
                    return at < 0 ? -1 : s + lo + at;
                });
        } else {
            for (int p = t; p < n; p += lanes) {
                cols[p] = a.C.col[s + p];
                cv[p] = a.C.val[s + p];
            }
            sub_staged<VAL_GROUP, S, PASS>(
                a, a0, ae, t, lanes, d, sync,
                [&](int c, V& x) {
                    const int slot = find_slot(cols, n, c);
                    if (slot >= 0) x = cv[slot];
                    return slot;
                },
                [&](int slot, int) { return s + slot; });
        }
    });
}

// Team class: VAL_TEAM_LANES lanes per row, the teams of a wave in step; a team's lanes are the group
// of each of its A entries.
template <class V, int SR, int PASS>
__global__ __launch_bounds__(256) void k_sub_team(ValSubArgs<V> a, const int* __restrict__ list, int count, int region) {
    using S = SrValue<SR>;
    extern __shared__ __align__(16) char lds[];
    const int team = threadIdx.x / VAL_TEAM_LANES, t = threadIdx.x % VAL_TEAM_LANES;
    const ValSlice<V> sl = search_slice<V, 1>(lds + (size_t)team * region, region);
    V* cv = sl.val;
    int* cols = sl.cols;
    const bool wa = PASS == 2 && a.dA != nullptr, wb = PASS == 2 && a.dB != nullptr;
    for (int base = blockIdx.x * VAL_TEAM_ROWS; base < count; base += gridDim.x * VAL_TEAM_ROWS) {
        int s, n, a0 = 0, nA = 0;
        const int row = val_team_row(a, list, count, base + team, sl.ne, s, n);
        if (n > 0) {
            a0 = a.A.ptr[row];
            nA = a.A.ptr[row + 1] - a0;
        }
        for (int p = t; p < n; p += VAL_TEAM_LANES) {
            cols[p] = a.C.col[s + p];
            cv[p] = a.C.val[s + p];
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
                const V av = a.A.val[a0 + it];
                const int be = a.B.ptr[ac + 1];
                for (int j = a.B.ptr[ac] + t; j < be; j += VAL_TEAM_LANES) {
                    const int slot = find_slot(cols, n, a.B.col[j]);
                    if (slot >= 0) {
                        const V bv = a.B.val[j];
                        if (S::wins(av, bv, cv[slot])) sub_winner<S, PASS>(a, wa, wb, j, s + slot, av, bv, sum, ac);
                    }
                }
            }
            if (wa) sub_store<VAL_TEAM_LANES>(a, on, t, a0 + it, sum);
        }
        vwave_sync();
    }
}

// Wave classes: one wave64 per row, WPB rows per block.
template <class V, int SR, int PASS, bool DIRECT>
__global__ __launch_bounds__(256) void k_sub_wave(ValSubArgs<V> a, const int* __restrict__ list, int count, int region) {
    extern __shared__ __align__(16) char lds[];
    __shared__ ValStage<64, V, 1> stage[WPB];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    auto sync = [] { vwave_sync(); };
    for (int idx = blockIdx.x * WPB + wave; idx < count; idx += gridDim.x * WPB)
        sub_row<DIRECT, SrValue<SR>, PASS>(a, list[idx], lds + (size_t)wave * region, region, lane, 64, stage[wave], sync);
}

// Block classes: one block of T threads per row, the forward's split of the list over the XCDs.
template <class V, int SR, int PASS, int T, bool DIRECT>
__global__ __launch_bounds__(T) void k_sub_block(ValSubArgs<V> a, const int* __restrict__ list, int count, int region) {
    extern __shared__ __align__(16) char lds[];
    __shared__ ValStage<VAL_STAGE, V, 1> stage;
    auto sync = [] { __syncthreads(); };
    const XcdStretch x = xcd_stretch(count);
    for (int idx = x.begin; idx < x.end; idx += x.step)
        sub_row<DIRECT, SrValue<SR>, PASS>(a, list[idx], lds, region, threadIdx.x, T, stage, sync);
}

// Global form, as k_grad_global: LANES lanes per row (1024: a block per row of the global class; 64: a wave per row,
// the dot rows of a masked plan).  C.col is searched and Cval read in HBM; nothing is staged.
template <class V, int SR, int PASS, int LANES>
__global__ __launch_bounds__(LANES < 256 ? 256 : LANES) void k_sub_global(ValSubArgs<V> a, const int* __restrict__ list,
                                                                          int count) {
    using S = SrValue<SR>;
    constexpr int THREADS = LANES < 256 ? 256 : LANES, ROWS = THREADS / LANES, NG = LANES / VAL_GROUP;
    const int t = threadIdx.x % LANES, g = t / VAL_GROUP, tl = t % VAL_GROUP;
    const bool wa = PASS == 2 && a.dA != nullptr, wb = PASS == 2 && a.dB != nullptr;
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
                const V av = a.A.val[k];
                const int be = a.B.ptr[ac + 1];
                for (int j = a.B.ptr[ac] + tl; j < be; j += VAL_GROUP) {
                    const int slot = find_slot(a.C.col + s, n, a.B.col[j]);
                    if (slot >= 0) {
                        const V bv = a.B.val[j];
                        if (S::wins(av, bv, a.C.val[s + slot])) sub_winner<S, PASS>(a, wa, wb, j, s + slot, av, bv, sum, ac);
                    }
                }
            }
            if (wa) sub_store<VAL_GROUP>(a, on, tl, k, sum);
        }
    }
}

// The subgradient's kernels over the LDS classes' lists (val_lds_kernel), for the value type, the semiring and the pass
template <class V, int SR, int PASS>
struct SubKernels {
    using Fn = void (*)(ValSubArgs<V>, const int*, int, int);
    static Fn team() { return k_sub_team<V, SR, PASS>; }
    template <bool DIRECT>
    static Fn wave() { return k_sub_wave<V, SR, PASS, DIRECT>; }
    template <int T, bool DIRECT>
    static Fn block() { return k_sub_block<V, SR, PASS, T, DIRECT>; }
};

// The stages are the plus-times backward's at width 1: val_static_lds is these kernels' static LDS too
template <class V>
constexpr bool sub_static_lds_holds() {
    return sizeof(ValStage<64, V, 1>[WPB]) == val_static_lds(VK_WAVE_DIRECT, sizeof(V), 1) &&
           sizeof(ValStage<VAL_STAGE, V, 1>) == val_static_lds(VK_BLOCK_SEARCH, sizeof(V), 1);
}
static_assert(sub_static_lds_holds<double>() && sub_static_lds_holds<float>(), "val_static_lds is the subgradient kernels' static LDS");
// (at width 1 no team launch is past what a launch may take unasked: only the block kernels are registered)
static_assert(!val_team_registers(VAL_VB_F64) && !val_team_registers(VAL_VB_F32), "the team kernels need no attribute");

template <class V, int SR>
hipError_t sub_register() {
    hipError_t e = val_allow_max_lds<SubKernels<V, SR, 1>>();
    if (e == hipSuccess) e = val_allow_max_lds<SubKernels<V, SR, 2>>();
    return e == hipSuccess ? val_allow_max_lds<SubKernels<V, SR, 3>>() : e;
}
template <class V>
hipError_t sub_register_semirings() {
    hipError_t e = sub_register<V, SR_MIN_PLUS>();
    if (e == hipSuccess) e = sub_register<V, SR_MAX_PLUS>();
    if (e == hipSuccess) e = sub_register<V, SR_MAX_MIN>();
    return e;
}

template <class V, int SR, int PASS>
void issue_sub(const ValLaunch& l, const ValSubArgs<V>& a, const int* list, hipStream_t s) {
    const dim3 g(l.grid), b(l.block);
    if (const typename SubKernels<V, SR, PASS>::Fn k = val_lds_kernel<SubKernels<V, SR, PASS>>(l.kernel, l.block)) {
        hipLaunchKernelGGL(k, g, b, l.lds, s, a, list, l.count, l.region);
    } else if (l.kernel == VK_GLOBAL) {  // (plan_grad has no other kernel)
        // 1024 threads a row for the global class, a wave a row for the dot rows
        if (l.block == 1024) hipLaunchKernelGGL((k_sub_global<V, SR, PASS, 1024>), g, b, 0, s, a, list, l.count);
        else hipLaunchKernelGGL((k_sub_global<V, SR, PASS, 64>), g, b, 0, s, a, list, l.count);
    }
}
template <class V, int SR>
void issue_sub_pass(const ValLaunch& l, int pass, const ValSubArgs<V>& a, const int* list, hipStream_t s) {
    if (pass == 1) issue_sub<V, SR, 1>(l, a, list, s);
    else if (pass == 2) issue_sub<V, SR, 2>(l, a, list, s);
    else if (pass == 3) issue_sub<V, SR, 3>(l, a, list, s);
}

}  // namespace

hipError_t init_values_subgrad_attributes() {
    const hipError_t e = sub_register_semirings<double>();
    return e == hipSuccess ? sub_register_semirings<float>() : e;
}

template <class V>
void issue_values_subgrad(const ValLaunch& l, int semiring, int pass, const ValSubArgs<V>& a, const int* list, hipStream_t s) {
    switch (semiring) {  // (plus-times has a gradient, mhs_values_grad.hip: nothing to launch here)
    case SR_MIN_PLUS: return issue_sub_pass<V, SR_MIN_PLUS>(l, pass, a, list, s);
    case SR_MAX_PLUS: return issue_sub_pass<V, SR_MAX_PLUS>(l, pass, a, list, s);
    case SR_MAX_MIN: return issue_sub_pass<V, SR_MAX_MIN>(l, pass, a, list, s);
    }
}
template void issue_values_subgrad<double>(const ValLaunch&, int, int, const ValSubArgs<double>&, const int*, hipStream_t);
template void issue_values_subgrad<float>(const ValLaunch&, int, int, const ValSubArgs<float>&, const int*, hipStream_t);

}  // namespace mhs
