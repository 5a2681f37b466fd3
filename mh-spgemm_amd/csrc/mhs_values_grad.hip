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
// dB: one global_atomic_add_f64 per kept product into the zero-filled dB; a group's lanes hit
// consecutive entries of one B row.  Which sides are wanted is a wave-uniform flag (the output's pointer):
// a dA-only call issues no atomic and reads no Aval, a dB-only call reads no Bval.
#include "mhs_valwalk.hpp"

namespace mhs {
namespace {

// Sum over the G lanes of a group (a power of two); every lane of the group must be here.
template <int G>
__device__ __forceinline__ double group_sum(double v) {
#pragma unroll
    for (int m = G / 2; m > 0; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

// One kept product: B entry q, cotangent gv; sum is the lane's share of the A entry's gradient.
__device__ __forceinline__ void grad_product(const ValGradArgs& a, bool wa, bool wb, int q, double bv, double av, double gv,
                                             double& sum) {
    if (wa) sum += bv * gv;
    if (wb) unsafeAtomicAdd(&a.dB[q], av * gv);  // global_atomic_add_f64
}

// The staged walk of walk_staged (mhs_values.hip) for a wave's or a block's row, backwards.  The row's
// `lanes` lanes stage up to CH A entries; group g of ng then takes staged entries g, g + ng, ... in
// steps all groups make together, reads its B row VAL_PIECES G-wide pieces at a time, and asks
// look(column, gv) for the cotangent of each product (false: not in the row).  sync() publishes the
// caller's staging of G with the first stage.
template <int G, int CH, class Sync, class Look>
__device__ __forceinline__ void grad_staged(const ValGradArgs& a, int a0, int ae, int t, int lanes, ValStage<CH>& d, Sync sync,
                                            Look look) {
    const int g = t / G, ng = lanes / G, tl = t % G;
    const bool wa = a.dA != nullptr, wb = a.dB != nullptr;
    for (int k0 = a0; k0 < ae; k0 += CH) {
        const int cnt = ae - k0 < CH ? ae - k0 : CH;
        if (t < cnt) {
            const int ac = a.Acol[k0 + t];
            const int bs = a.Bptr[ac];
            d.bs[t] = bs;
            d.len[t] = a.Bptr[ac + 1] - bs;
            d.av[t] = wb ? a.Aval[k0 + t] : 0.0;
        }
        sync();
        for (int e0 = 0; e0 < cnt; e0 += ng) {  // the same trip count in every lane of the row
            const int e = e0 + g;
            const bool on = e < cnt;
            double sum = 0.0;
            if (on) {
                const int bs = d.bs[e], len = d.len[e];
                const double av = d.av[e];
                for (int j = tl; j < len; j += VAL_PIECES * G) {
                    int c[VAL_PIECES];
                    double v[VAL_PIECES];
#pragma unroll
                    for (int u = 0; u < VAL_PIECES; ++u) {
                        const int jj = j + u * G;
                        const bool in = jj < len;
                        c[u] = in ? a.Bcol[bs + jj] : -1;
                        v[u] = in && wa ? a.Bval[bs + jj] : 0.0;
                    }
#pragma unroll
                    for (int u = 0; u < VAL_PIECES; ++u) {
                        double gv;
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

// One row of a wave or block class: stage G (and C.col) in the row's LDS slice, then the walk.
template <bool DIRECT, int CH, class Sync>
__device__ __forceinline__ void grad_row(const ValGradArgs& a, int row, int s, int n, int first, int span, double* g, int* cols,
                                         int t, int lanes, ValStage<CH>& d, Sync sync) {
    const int a0 = a.Aptr[row], ae = a.Aptr[row + 1];
    if (a0 >= ae) return;
    if constexpr (DIRECT) {
        for (int p = t; p < span; p += lanes) g[p] = 0.0;
        sync();
        for (int p = t; p < n; p += lanes) g[a.Ccol[s + p] - first] = a.G[s + p];
        grad_staged<VAL_GROUP>(a, a0, ae, t, lanes, d, sync, [&](int c, double& gv) {
            const unsigned slot = (unsigned)(c - first);
            if (slot >= (unsigned)span) return false;
            gv = g[slot];
            return gv != 0.0;  // (0: outside the pattern, or a zero cotangent -- nothing to add either way)
        });
    } else {
        for (int p = t; p < n; p += lanes) {
            cols[p] = a.Ccol[s + p];
            g[p] = a.G[s + p];
        }
        grad_staged<VAL_GROUP>(a, a0, ae, t, lanes, d, sync, [&](int c, double& gv) {
            const int slot = find_slot(cols, n, c);
            if (slot < 0) return false;
            gv = g[slot];
            return true;
        });
    }
}

// Team class: VAL_TEAM_LANES lanes per row, the teams of a wave in step; a team's lanes are the group
// of each of its A entries.
__global__ __launch_bounds__(256) void k_grad_team(ValGradArgs a, const int* __restrict__ list, int count, int region) {
    extern __shared__ __align__(16) char lds[];
    const int team = threadIdx.x / VAL_TEAM_LANES, t = threadIdx.x % VAL_TEAM_LANES;
    const int ne = region / 12;
    double* g = (double*)(lds + (size_t)team * region);
    int* cols = (int*)(g + ne);
    const bool wa = a.dA != nullptr, wb = a.dB != nullptr;
    for (int base = blockIdx.x * VAL_TEAM_ROWS; base < count; base += gridDim.x * VAL_TEAM_ROWS) {
        const int idx = base + team;
        const int row = idx < count ? list[idx] : -1;
        int s = 0, n = 0, a0 = 0, nA = 0;
        if (row >= 0) {
            s = a.Cptr[row];
            n = a.Cptr[row + 1] - s;
            if (n > ne) n = 0;  // (not this plan's pattern: leave the row alone rather than overrun the slice)
        }
        if (n > 0) {
            a0 = a.Aptr[row];
            nA = a.Aptr[row + 1] - a0;
        }
        for (int p = t; p < n; p += VAL_TEAM_LANES) {
            cols[p] = a.Ccol[s + p];
            g[p] = a.G[s + p];
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
            double sum = 0.0;
            if (on) {
                const int ac = a.Acol[a0 + it];
                const double av = wb ? a.Aval[a0 + it] : 0.0;
                const int be = a.Bptr[ac + 1];
                for (int j = a.Bptr[ac] + t; j < be; j += VAL_TEAM_LANES) {
                    const int slot = find_slot(cols, n, a.Bcol[j]);
                    if (slot >= 0) grad_product(a, wa, wb, j, wa ? a.Bval[j] : 0.0, av, g[slot], sum);
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
template <bool DIRECT>
__global__ __launch_bounds__(256) void k_grad_wave(ValGradArgs a, const int* __restrict__ list, int count, int region) {
    extern __shared__ __align__(16) char lds[];
    __shared__ ValStage<64> stage[WPB];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double* g = (double*)(lds + (size_t)wave * region);
    auto sync = [] { vwave_sync(); };
    for (int idx = blockIdx.x * WPB + wave; idx < count; idx += gridDim.x * WPB) {
        const int row = list[idx];
        const int s = a.Cptr[row], n = a.Cptr[row + 1] - s;
        if (n <= 0) continue;
        if constexpr (DIRECT) {
            const int first = a.Ccol[s];
            const long long span = (long long)a.Ccol[s + n - 1] - first + 1;
            if (span <= 0 || span * 8 > region) continue;  // (not this plan's pattern)
            grad_row<true>(a, row, s, n, first, (int)span, g, nullptr, lane, 64, stage[wave], sync);
        } else {
            const int ne = region / 12;
            if (n > ne) continue;
            grad_row<false>(a, row, s, n, 0, 0, g, (int*)(g + ne), lane, 64, stage[wave], sync);
        }
    }
}

// Block classes: one block of T threads per row, the forward's split of the list over the XCDs.
template <int T, bool DIRECT>
__global__ __launch_bounds__(T) void k_grad_block(ValGradArgs a, const int* __restrict__ list, int count, int region) {
    extern __shared__ __align__(16) char lds[];
    __shared__ ValStage<VAL_STAGE> stage;
    double* g = (double*)lds;
    const int t = threadIdx.x;
    auto sync = [] { __syncthreads(); };
    int lo = 0, hi = count, first_j = blockIdx.x, step = gridDim.x;
    if (gridDim.x >= 8) {
        const int xcd = blockIdx.x & 7;
        int before = 0;
        for (int y = 0; y < xcd; ++y) before += (gridDim.x - y + 7) >> 3;
        step = (gridDim.x - xcd + 7) >> 3;
        first_j = blockIdx.x >> 3;
        lo = (int)((long long)count * before / gridDim.x);
        hi = (int)((long long)count * (before + step) / gridDim.x);
    }
    for (int idx = lo + first_j; idx < hi; idx += step) {
        const int row = list[idx];
        const int s = a.Cptr[row], n = a.Cptr[row + 1] - s;
        if (n <= 0) continue;
        if constexpr (DIRECT) {
            const int first = a.Ccol[s];
            const long long span = (long long)a.Ccol[s + n - 1] - first + 1;
            if (span <= 0 || span * 8 > region) continue;
            grad_row<true>(a, row, s, n, first, (int)span, g, nullptr, t, T, stage, sync);
        } else {
            const int ne = region / 12;
            if (n > ne) continue;
            grad_row<false>(a, row, s, n, 0, 0, g, (int*)(g + ne), t, T, stage, sync);
        }
    }
}

// Global form: LANES lanes per row (1024: a block per row of the global class; 64: a wave per row, the
// dot rows of a masked plan, which the forward computes per mask entry and the backward walks by
// products -- right for any row, not tuned).  C.col is searched and G read in HBM; nothing is staged.
template <int LANES>
__global__ __launch_bounds__(LANES < 256 ? 256 : LANES) void k_grad_global(ValGradArgs a, const int* __restrict__ list, int count) {
    constexpr int THREADS = LANES < 256 ? 256 : LANES, ROWS = THREADS / LANES, NG = LANES / VAL_GROUP;
    const int t = threadIdx.x % LANES, g = t / VAL_GROUP, tl = t % VAL_GROUP;
    const bool wa = a.dA != nullptr, wb = a.dB != nullptr;
    for (int idx = blockIdx.x * ROWS + threadIdx.x / LANES; idx < count; idx += gridDim.x * ROWS) {
        const int row = list[idx];
        const int s = a.Cptr[row], n = a.Cptr[row + 1] - s;
        if (n <= 0) continue;
        const int a0 = a.Aptr[row], ae = a.Aptr[row + 1];
        for (int k0 = a0; k0 < ae; k0 += NG) {  // the same trip count in every lane of the row
            const int k = k0 + g;
            const bool on = k < ae;
            double sum = 0.0;
            if (on) {
                const int ac = a.Acol[k];
                const double av = wb ? a.Aval[k] : 0.0;
                const int be = a.Bptr[ac + 1];
                for (int j = a.Bptr[ac] + tl; j < be; j += VAL_GROUP) {
                    const int slot = find_slot(a.Ccol + s, n, a.Bcol[j]);
                    if (slot >= 0) grad_product(a, wa, wb, j, wa ? a.Bval[j] : 0.0, av, a.G[s + slot], sum);
                }
            }
            if (wa) {
                sum = group_sum<VAL_GROUP>(sum);
                if (on && tl == 0) a.dA[k] = sum;
            }
        }
    }
}

}  // namespace

hipError_t init_values_grad_attributes() {
    // as the forward's: the 1024-thread block kernels may take the whole 160 KiB
    hipError_t e = hipFuncSetAttribute((const void*)k_grad_block<1024, true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       VAL_BLOCK_BYTES);
    if (e == hipSuccess)
        e = hipFuncSetAttribute((const void*)k_grad_block<1024, false>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                VAL_BLOCK_BYTES);
    return e;
}

void issue_values_grad(const ValLaunch& l, const ValGradArgs& a, const int* list, hipStream_t s) {
    const dim3 g(l.grid), b(l.block);
    switch (l.kernel) {
    case VK_TEAM: hipLaunchKernelGGL(k_grad_team, g, b, l.lds, s, a, list, l.count, l.region); break;
    case VK_WAVE_DIRECT: hipLaunchKernelGGL(k_grad_wave<true>, g, b, l.lds, s, a, list, l.count, l.region); break;
    case VK_WAVE_SEARCH: hipLaunchKernelGGL(k_grad_wave<false>, g, b, l.lds, s, a, list, l.count, l.region); break;
    case VK_BLOCK_DIRECT:
        if (l.block == 1024) hipLaunchKernelGGL((k_grad_block<1024, true>), g, b, l.lds, s, a, list, l.count, l.region);
        else hipLaunchKernelGGL((k_grad_block<256, true>), g, b, l.lds, s, a, list, l.count, l.region);
        break;
    case VK_BLOCK_SEARCH:
        if (l.block == 1024) hipLaunchKernelGGL((k_grad_block<1024, false>), g, b, l.lds, s, a, list, l.count, l.region);
        else hipLaunchKernelGGL((k_grad_block<256, false>), g, b, l.lds, s, a, list, l.count, l.region);
        break;
    case VK_GLOBAL:  // (plan_grad: 1024 threads a row for the global class, a wave a row for the dot rows)
        if (l.block == 1024) hipLaunchKernelGGL(k_grad_global<1024>, g, b, 0, s, a, list, l.count);
        else hipLaunchKernelGGL(k_grad_global<64>, g, b, 0, s, a, list, l.count);
        break;
    default: break;  // (plan_grad has no other kernel)
    }
}

}  // namespace mhs
