// mhs_values_smooth.hip -- the smoothed values plans (mhs_values_plan_create_smooth): the forward of a min-plus or
// max-plus plan whose reduce is log-sum-exp, and its gradient (mhs_spgemm_values_softgrad), at width 1.
//
// The value-level rule is mhs_smooth.hpp: the kernels work on the signed products v = sg * (a + b) (sg = +1 under
// max-plus, -1 under min-plus: a kernel argument), reduce them as under max-plus and hand sg * result out.
//
// Forward.  The plan is classified at twice the value's bytes, so a row's LDS slice holds two planes laid out as a
// width-2 plan's sums: acc[0 * pitch + slot] the entry's running max, acc[1 * pitch + slot] its sum.  Per row of a
// team, wave or block class, in the row frame of mhs_valwalk.hpp:
//   1  the max plane filled with -Inf, the sum plane with 0 (search: the row's C.col staged behind them) -- on the
//      first stage's sync
//   2  the products walked: ds_max of v into the max plane              3  sync
//   4  the products walked again: ds_add of exp(v - M[slot]) into the sum plane -- the second walk reads the row's A
//      and B entries again (from L2, mostly); nothing of the first walk is kept              5  sync
//   6  every entry stored: sg * finish(M, sum)
//   dot (masked plans)   a lane per mask entry, as k_val_dot: two sweeps over A's row, max then sum, in registers, in
//                        A's entry order then B's duplicate order -- no atomics, the same bits on every call
//   global               no second plane and no scratch: the row's Cval segment filled with the identity, then every
//                        product replaces its entry c by sg * logaddexp(sg * c, v) in a compare-and-swap loop
// exp, log and log1p are the precise ones of the device library.
//
// Gradient.  One pass of the plan's backward launch list, the backward walk of mhs_backwalk.hpp: the two planes of the
// row's slice hold G and sg * Cval, staged the same way; per kept product one slot lookup, two LDS reads and one exp
// give w = G[s] * exp(v - sg * Cval[s]) (Smooth::weight: exactly 0 where Cval[s] is not finite), which feeds the
// register sum of its A entry -- reduced across the lane group by shuffles and stored once, in a fixed order -- and goes
// to dB[q] by one unsafeAtomicAdd.  In the direct classes the Cval plane is filled with NaN over the span, so a column
// outside the pattern has weight 0 (the subgradient's trick).  The global form (the global class, and a masked plan's
// dot rows) searches C.col and reads G and Cval in HBM.
#include "mhs_backwalk.hpp"
#include "mhs_smooth.hpp"

#include <type_traits>

namespace mhs {
namespace {

// The reduce of a product into its entry's planes: ds_max_f64 / ds_max_f32, ds_add_f64 / ds_add_f32
template <class V>
__device__ __forceinline__ void soft_lds_max(V* p, V v) {
    (void)__hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
template <class V>
__device__ __forceinline__ void soft_lds_add(V* p, V v) {
    atomicAdd(p, v);
}
// ... and into its entry of Cval (the global class): c <- sg * logaddexp(sg * c, v), until no other product came between
template <class V>
__device__ __forceinline__ void soft_glob(V* p, V v, V sg) {
    using U = typename std::conditional<sizeof(V) == 8, unsigned long long, unsigned>::type;
    U* up = (U*)p;
    U old = __hip_atomic_load(up, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (;;) {
        const V next = sg * Smooth<V>::logaddexp(sg * __builtin_bit_cast(V, old), v);
        const U nu = __builtin_bit_cast(U, next);
        if (nu == old) return;  // (an identity product, or a NaN that is there already)
        if (__hip_atomic_compare_exchange_strong(up, &old, nu, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
    }
}

// ----------------------------------------------------------------- forward ---
// The signed products of a row are the forward's walks (walk_products and walk_staged of mhs_valwalk.hpp) at width 1
// under max-plus, whose product is the one rounding of a + b, with the sign applied in the callback: sg * (a + b) is
// Smooth<V>::mul(sg, a, b) to the bit, a multiplication by +-1 being exact.  f(column, v) per product.
using MaxPlus = SrPolicy<SR_MAX_PLUS>;
template <class V, class F>
__device__ __forceinline__ auto soft_signed(V sg, F f) {
    return [=](int c, const ValSums<V, 1>& p) { f(c, sg * p.x[0]); };
}

// One row of a wave or block class in the row frame, guarded at two planes of V: steps 1 to 6 of the header.
template <bool DIRECT, int CH, class V, class Sync>
__device__ __forceinline__ void soft_row(const ValArgs<V>& a, V sg, int row, char* base, int region, int t, int lanes,
                                         ValStage<CH, V, 1>& d, Sync sync) {
    val_row<DIRECT, 2>(a, row, base, region, [&](int s, int n, int first, int span, V* acc, int* cols) {
        // the pitch of the planes: the span, or the slice's entries (as search_slice)
        const int pitch = DIRECT ? span : val_slice_entries(region, 2 * (int)sizeof(V));
        V* mx = acc;
        V* sm = acc + pitch;
        auto slot_of = [&](int c) {
            if constexpr (DIRECT) {
                const unsigned slot = (unsigned)(c - first);
                return slot < (unsigned)span ? (int)slot : -1;
            } else {
                return find_slot(cols, n, c);
            }
        };
        walk_staged<VAL_GROUP, 1, MaxPlus>(
            a, row, t, lanes, d, sync,
            [&] {
                for (int p = t; p < (DIRECT ? span : n); p += lanes) {
                    if constexpr (!DIRECT) cols[p] = a.C.col[s + p];
                    mx[p] = Smooth<V>::floor();
                    sm[p] = V(0);
                }
            },
            soft_signed(sg, [&](int c, V v) {
                const int slot = slot_of(c);
                if (slot >= 0) soft_lds_max(&mx[slot], v);
            }));
        walk_staged<VAL_GROUP, 1, MaxPlus>(
            a, row, t, lanes, d, sync, [] {},
            soft_signed(sg, [&](int c, V v) {
                const int slot = slot_of(c);
                if (slot >= 0) soft_lds_add(&sm[slot], Smooth<V>::term(v, mx[slot]));
            }));
        for (int p = t; p < n; p += lanes) {
            const int slot = DIRECT ? a.C.col[s + p] - first : p;
            a.C.val[s + p] = sg * Smooth<V>::finish(mx[slot], sm[slot]);
        }
        sync();
    });
}

// Team class: VAL_TEAM_LANES lanes per row, the teams of a wave in step (wave-level ordering).
template <class V>
__global__ __launch_bounds__(256) void k_soft_team(ValArgs<V> a, V sg, const int* __restrict__ list, int count, int region) {
    extern __shared__ __align__(16) char lds[];
    const int team = threadIdx.x / VAL_TEAM_LANES, t = threadIdx.x % VAL_TEAM_LANES;
    const ValSlice<V> sl = search_slice<V, 2>(lds + (size_t)team * region, region);
    V* mx = sl.val;
    V* sm = sl.val + sl.ne;
    int* cols = sl.cols;
    for (int base = blockIdx.x * VAL_TEAM_ROWS; base < count; base += gridDim.x * VAL_TEAM_ROWS) {
        int s, n;
        const int row = val_team_row(a, list, count, base + team, sl.ne, s, n);
        for (int p = t; p < n; p += VAL_TEAM_LANES) {
            cols[p] = a.C.col[s + p];
            mx[p] = Smooth<V>::floor();
            sm[p] = V(0);
        }
        vwave_sync();
        if (n > 0)
            walk_products<VAL_TEAM_LANES, 1, MaxPlus>(a, row, 0, 1, t, soft_signed(sg, [&](int c, V v) {
                const int slot = find_slot(cols, n, c);
                if (slot >= 0) soft_lds_max(&mx[slot], v);
            }));
        vwave_sync();
        if (n > 0)
            walk_products<VAL_TEAM_LANES, 1, MaxPlus>(a, row, 0, 1, t, soft_signed(sg, [&](int c, V v) {
                const int slot = find_slot(cols, n, c);
                if (slot >= 0) soft_lds_add(&sm[slot], Smooth<V>::term(v, mx[slot]));
            }));
        vwave_sync();
        for (int p = t; p < n; p += VAL_TEAM_LANES) a.C.val[s + p] = sg * Smooth<V>::finish(mx[p], sm[p]);
        vwave_sync();
    }
}

// Wave classes: one wave64 per row, WPB rows per block.
template <class V, bool DIRECT>
__global__ __launch_bounds__(256) void k_soft_wave(ValArgs<V> a, V sg, const int* __restrict__ list, int count, int region) {
    extern __shared__ __align__(16) char lds[];
    __shared__ ValStage<64, V, 1> stage[WPB];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    auto sync = [] { vwave_sync(); };
    for (int idx = blockIdx.x * WPB + wave; idx < count; idx += gridDim.x * WPB)
        soft_row<DIRECT>(a, sg, list[idx], lds + (size_t)wave * region, region, lane, 64, stage[wave], sync);
}

// Block classes: one block of T threads per row, up to the whole 160 KiB (VAL_BLOCK_BYTES dynamic + the stage).
template <class V, int T, bool DIRECT>
__global__ __launch_bounds__(T) void k_soft_block(ValArgs<V> a, V sg, const int* __restrict__ list, int count, int region) {
    extern __shared__ __align__(16) char lds[];
    __shared__ ValStage<VAL_STAGE, V, 1> stage;
    auto sync = [] { __syncthreads(); };
    const XcdStretch x = xcd_stretch(count);
    for (int idx = x.begin; idx < x.end; idx += x.step) soft_row<DIRECT>(a, sg, list[idx], lds, region, threadIdx.x, T, stage, sync);
}

// Global class: the row's Cval segment is the accumulator.
template <class V>
__global__ __launch_bounds__(1024) void k_soft_global(ValArgs<V> a, V sg, const int* __restrict__ list, int count) {
    const int t = threadIdx.x;
    for (int idx = blockIdx.x; idx < count; idx += gridDim.x) {
        const int row = list[idx];
        const int s = a.C.ptr[row], n = a.C.ptr[row + 1] - s;
        for (int p = t; p < n; p += 1024) a.C.val[s + p] = sg * Smooth<V>::floor();
        __threadfence();
        __syncthreads();
        walk_products<VAL_GROUP, 1, MaxPlus>(a, row, t / VAL_GROUP, 1024 / VAL_GROUP, t % VAL_GROUP, soft_signed(sg, [&](int c, V v) {
            const int slot = find_slot(a.C.col + s, n, c);
            if (slot >= 0) soft_glob(&a.C.val[s + slot], v, sg);
        }));
    }
}

// Dot class (masked plans): one wave64 per row, WPB rows per block, lane l owning the mask entries l, l + 64, ... as
// in k_val_dot.  sweep(f) visits the entry's products in A's entry order, then B's duplicate order: once for the max,
// once for the sum.
template <class V>
struct SoftDotStage {
    int col[64];
    V av[64];
};
template <class V>
__global__ __launch_bounds__(256) void k_soft_dot(ValArgs<V> a, V sg, ValTrans tr, const int* __restrict__ list, int count) {
    __shared__ SoftDotStage<V> stage[WPB];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    SoftDotStage<V>& d = stage[wave];
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
            auto sweep = [&](auto f) {
                for (int k0 = a0; k0 < ae; k0 += 64) {
                    const int cnt = ae - k0 < 64 ? ae - k0 : 64;
                    if (lane < cnt) {
                        d.col[lane] = a.A.col[k0 + lane];
                        d.av[lane] = a.A.val[k0 + lane];
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
                            for (; lo < hi0 && tr.trow[lo] == ac; ++lo) f(Smooth<V>::mul(sg, d.av[e], a.B.val[tr.tperm[lo]]));
                        }
                    vwave_sync();
                }
            };
            V M = Smooth<V>::floor(), sum = V(0);
            sweep([&](V v) { M = Smooth<V>::max(M, v); });
            sweep([&](V v) { sum += Smooth<V>::term(v, M); });
            if (p < n) a.C.val[s + p] = sg * Smooth<V>::finish(M, sum);
        }
    }
}

template <class V>
struct SoftKernels {
    using Fn = void (*)(ValArgs<V>, V, const int*, int, int);
    static Fn team() { return k_soft_team<V>; }
    template <bool DIRECT>
    static Fn wave() { return k_soft_wave<V, DIRECT>; }
    template <int T, bool DIRECT>
    static Fn block() { return k_soft_block<V, T, DIRECT>; }
};

// ---------------------------------------------------------------- gradient ---
// The smoothed gradient's rule of the backward walk (mhs_backwalk.hpp), at width 1: two planes, G (0 outside the
// pattern) and sg * Cval (NaN outside it: no weight); both operands are read always.
template <class V_>
struct SoftRule {
    using V = V_;
    using Args = ValSoftArgs<V>;
    static constexpr int PLANES = 2;
    static __device__ __forceinline__ BackWants wants(const Args& a) { return {a.dA != nullptr, a.dB != nullptr}; }
    static __device__ __forceinline__ V staged(const Args& a, int pl, int pos) { return pl == 0 ? a.G[pos] : a.sg * a.C.val[pos]; }
    static __device__ __forceinline__ V fill(int pl) { return pl == 0 ? V(0) : std::numeric_limits<V>::quiet_NaN(); }

    // One kept product: B entry q, its signed value v, its entry's cotangent g and signed result c; sum is the lane's
    // share of the A entry's gradient.
    static __device__ __forceinline__ void soft_product(const Args& a, BackWants f, int q, V v, V c, V g, V& sum) {
        const V w = Smooth<V>::weight(v, c, g);
        if (f.wa) sum += w;
        if (f.wb && w != V(0)) unsafeAtomicAdd(a.dB + q, w);  // global_atomic_add_f64 / _f32 (a NaN weight is added)
    }
    template <int P, class Row>
    static __device__ __forceinline__ void pieces(const Args& a, BackWants f, const Row& row, int q, int, const int (&c)[P],
                                                  const V (&v)[P], V av, V& sum) {
#pragma unroll
        for (int u = 0; u < P; ++u) {
            const int slot = c[u] >= 0 ? row.slot(c[u]) : -1;
            if (slot < 0) continue;
            const V cv = row.at(1, slot);
            // (direct: NaN outside the pattern, and a result that is not finite, have no weight)
            if (Row::direct && !Smooth<V>::finite(cv)) continue;
            soft_product(a, f, q + u * VAL_GROUP, Smooth<V>::mul(a.sg, av, v[u]), cv, row.at(0, slot), sum);
        }
    }
    template <class Src>
    static __device__ __forceinline__ void product(const Args& a, BackWants f, int q, int, V av, const Src& src, int slot, V& sum) {
        soft_product(a, f, q, Smooth<V>::mul(a.sg, av, a.B.val[q]), src.at(1, slot), src.at(0, slot), sum);
    }
};

// The forward's stages are the width-1 kernels': val_static_lds at (vb, width 1) is these kernels' static LDS, beside
// launches planned at twice the value's bytes (tests/valplan_smooth_check.cpp sums the two)
template <class V>
constexpr bool soft_static_lds_holds() {
    return sizeof(ValStage<64, V, 1>[WPB]) == val_static_lds(VK_WAVE_DIRECT, sizeof(V), 1) &&
           sizeof(ValStage<VAL_STAGE, V, 1>) == val_static_lds(VK_BLOCK_SEARCH, sizeof(V), 1) &&
           sizeof(SoftDotStage<V>[WPB]) == val_static_lds(VK_DOT, sizeof(V), 1);
}
static_assert(soft_static_lds_holds<double>() && soft_static_lds_holds<float>(), "val_static_lds is the smoothed kernels' static LDS");
// (at two planes no team launch is past what a launch may take unasked: only the forward's block kernels are registered)
static_assert(!val_team_registers(2 * VAL_VB_F64) && !val_team_registers(2 * VAL_VB_F32), "the team kernels need no attribute");

template <class V>
hipError_t soft_register() {
    const hipError_t e = val_allow_max_lds<SoftKernels<V>>();
    return e == hipSuccess ? back_register<SoftRule<V>>() : e;
}

}  // namespace

hipError_t init_values_smooth_attributes() {
    const hipError_t e = soft_register<double>();
    return e == hipSuccess ? soft_register<float>() : e;
}

template <class V>
void issue_values_smooth(const ValLaunch& l, int semiring, const ValArgs<V>& a, const ValTrans& t, const int* list, hipStream_t s) {
    if (!val_smooth_serves(semiring)) return;
    const V sg = V(val_smooth_sign(semiring));
    const dim3 g(l.grid), b(l.block);
    if (const typename SoftKernels<V>::Fn k = val_lds_kernel<SoftKernels<V>>(l.kernel, l.block)) {
        hipLaunchKernelGGL(k, g, b, l.lds, s, a, sg, list, l.count, l.region);
    } else if (l.kernel == VK_GLOBAL) {
        hipLaunchKernelGGL((k_soft_global<V>), g, b, 0, s, a, sg, list, l.count);
    } else if (l.kernel == VK_DOT) {
        hipLaunchKernelGGL((k_soft_dot<V>), g, b, 0, s, a, sg, t, list, l.count);
    }
}
template void issue_values_smooth<double>(const ValLaunch&, int, const ValArgs<double>&, const ValTrans&, const int*, hipStream_t);
template void issue_values_smooth<float>(const ValLaunch&, int, const ValArgs<float>&, const ValTrans&, const int*, hipStream_t);

template <class V>
void issue_values_softgrad(const ValLaunch& l, int semiring, const ValSoftArgs<V>& args, const int* list, hipStream_t s) {
    if (!val_smooth_serves(semiring)) return;
    ValSoftArgs<V> a = args;
    a.sg = V(val_smooth_sign(semiring));
    back_issue<SoftRule<V>>(l, a, list, s);
}
template void issue_values_softgrad<double>(const ValLaunch&, int, const ValSoftArgs<double>&, const int*, hipStream_t);
template void issue_values_softgrad<float>(const ValLaunch&, int, const ValSoftArgs<float>&, const int*, hipStream_t);

}  // namespace mhs
