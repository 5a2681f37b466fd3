// mhs_values_subgrad.hip -- the subgradient of a semiring values plan (mhs_spgemm_values_subgrad): the backward of
// (Aval, Bval) -> Cval under min-plus, max-plus and max-min on a kept plan, at width 1.
//
// The rule (include/mhspgemm.h): a kept product (A entry p, B entry q, C slot s) is a winner of s when
// mul(Aval[p], Bval[q]) == Cval[s] and Cval[s] is not the identity of add (SrValue<SR>::wins); ties[s] counts the
// winners of s; each carries w = G[s] / ties[s], handed to dA[p] and dB[q] by the gradient of mul (share_a, share_b).
// The forward is bit-identical to a sequential evaluation and mul is formed here with the same one rounding, so the
// comparison is an equality of values, and every reached entry that is neither NaN nor the identity has a winner.
//
// It is the backward walk (mhs_backwalk.hpp) over the same launch list as the plus-times backward, twice: the row
// frame, the stage of A entries, the lane groups, the slice guards and the static LDS are that walk's.  The one LDS
// plane holds Cval -- the winner test is what every product needs, the cotangent only what a winner needs, and winners
// number about nnz(C):
//   team, wave-search, block-search   the row's C.col staged, its Cval segment beside it; a winner's position is s + slot
//   wave-direct, block-direct         c[col - first] over the span filled with NaN: a column outside the pattern
//                                     compares equal to nothing; a winner finds its position by find_slot in C.col + s
//                                     in memory, inside the few positions its place in the span leaves open
//   global (and a masked plan's dot rows)   C.col searched and Cval read in HBM
// Pass 1: every winner adds 1 to ties[position] (an integer global atomic without return).  Pass 2: every winner loads
// G and ties at its position, forms w, feeds the register sum of its A entry -- reduced across the lane group by
// shuffles and stored once, in a fixed order -- and adds its share to dB[q] by one unsafeAtomicAdd.
// In the wave and block walks a lane tests its VAL_PIECES pieces on LDS first and then takes its winners one after another.
// After staging LDS is read-only.  Which sides are wanted is a wave-uniform flag (the output's pointer).
//
// Pass 3 is the witness (mhs_spgemm_values_witness): the same walks and the same winner test once more, on their own
// call.  wit is filled with 0xFF bytes by the caller -- -1 as an int, the largest unsigned -- and every winner takes the
// unsigned minimum of its inner index k = A.col of its A entry into wit[position] (an integer global atomic without
// return): the smallest k among the winners, -1 where there is none, whatever the order.  It forms no weight, reduces
// nothing over the group and stores no gradient; the staged walk, whose stage keeps no column, reloads A.col for a
// winner (one address over the group).
#include "mhs_backwalk.hpp"

namespace mhs {
namespace {

// The subgradient's rule of the backward walk, for the value type, the semiring and the pass: one plane, Cval, NaN
// outside the pattern; both operands are read always; only pass 2 writes gradients, so passes 1 and 3 hold no group sum.
template <class V_, int SR, int PASS>
struct SubRule {
    using V = V_;
    using S = SrValue<SR>;
    using Args = ValSubArgs<V>;
    static constexpr int PLANES = 1;
    static __device__ __forceinline__ BackWants wants(const Args& a) {
        return {PASS == 2 && a.dA != nullptr, PASS == 2 && a.dB != nullptr};
    }
    static __device__ __forceinline__ V staged(const Args& a, int, int pos) { return a.C.val[pos]; }
    static __device__ __forceinline__ V fill(int) { return std::numeric_limits<V>::quiet_NaN(); }

    // One winner: B entry q, C position pos, its operands; sum is the lane's share of the A entry's gradient; k the
    // inner index of the product, the column of its A entry (read by pass 3 only).
    static __device__ __forceinline__ void winner(const Args& a, BackWants f, int q, int pos, V av, V bv, V& sum, int k) {
        if constexpr (PASS == 1) {
            (void)__hip_atomic_fetch_add(a.ties + pos, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // global_atomic_add_u32
        } else if constexpr (PASS == 3) {
            // wit is -1 = 0xFFFFFFFF until a winner comes: the unsigned minimum is the smallest k (k >= 0)
            // (a plain load of wit[pos] first, to skip the atomic where it is already <= k, was measured and lost: DESIGN 18)
            (void)__hip_atomic_fetch_min((unsigned*)a.wit + pos, (unsigned)k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // global_atomic_umin
        } else {
            const V w = a.G[pos] / V(a.ties[pos]);  // (ties >= 1: pass 1 counted this winner)
            if (f.wa) sum += S::share_a(av, bv, w);
            if (f.wb) {
                const V sb = S::share_b(av, bv, w);
                if (sb != V(0)) unsafeAtomicAdd(a.dB + q, sb);  // global_atomic_add_f64 / _f32 (a NaN share is added)
            }
        }
    }
    // The C position of a winner at `slot` of a staged row, its column c (-1: none)
    template <class Row>
    static __device__ __forceinline__ int where(const Args& a, const Row& row, int slot, int c) {
        if constexpr (Row::direct) {
            // C's columns ascend strictly: at most `slot` of them lie before column first + slot and at most
            // span - 1 - slot behind it, so its position is in [slot - (span - n), slot] -- on a dense row a
            // step or two of find_slot in C.col + s instead of log2(n)
            const int lo = slot - (row.span - row.n) > 0 ? slot - (row.span - row.n) : 0;
            const int hi = slot + 1 < row.n ? slot + 1 : row.n;
            const int at = find_slot(a.C.col + row.s + lo, hi - lo, c);
            return at < 0 ? -1 : row.s + lo + at;
        } else {
            return row.s + slot;
        }
    }
    template <int P, class Row>
    static __device__ __forceinline__ void pieces(const Args& a, BackWants f, const Row& row, int q, int k, const int (&c)[P],
                                                  const V (&v)[P], V av, V& sum) {
        // the winner test of the P pieces on LDS alone, then the lane's winners in ascending u: the wave
        // makes as many trips as its lane with the most winners, not P -- what a winner costs (its position,
        // the atomic, G and ties) is then paid about per winner, not per piece
        int h[P];
        V b[P];  // (the pieces' values, by value: the winners below pick theirs by a chain of selects on registers)
        unsigned left = 0;
#pragma unroll
        for (int u = 0; u < P; ++u) {
            b[u] = v[u];
            h[u] = c[u] >= 0 ? row.slot(c[u]) : -1;
            // (direct: NaN outside the pattern, no winner)
            if (h[u] >= 0 && S::wins(av, b[u], row.at(0, h[u]))) left |= 1u << u;
        }
        while (left) {
            const int u = __builtin_ctz(left);
            left &= left - 1;
            int hu = h[0], cu = c[0];
            V vu = b[0];
#pragma unroll
            for (int w = 1; w < P; ++w)
                if (u == w) hu = h[w], cu = c[w], vu = b[w];
            const int pos = where(a, row, hu, cu);
            // (the stage keeps no column: pass 3 reloads its A entry's, one address over the group)
            if (pos >= 0) winner(a, f, q + u * VAL_GROUP, pos, av, vu, sum, PASS == 3 ? a.A.col[k] : 0);
        }
    }
    template <class Src>
    static __device__ __forceinline__ void product(const Args& a, BackWants f, int q, int ac, V av, const Src& src, int slot, V& sum) {
        const V bv = a.B.val[q];
        if (S::wins(av, bv, src.at(0, slot))) winner(a, f, q, src.s + slot, av, bv, sum, ac);
    }
};

template <class V, int SR>
hipError_t sub_register() {
    hipError_t e = back_register<SubRule<V, SR, 1>>();
    if (e == hipSuccess) e = back_register<SubRule<V, SR, 2>>();
    return e == hipSuccess ? back_register<SubRule<V, SR, 3>>() : e;
}
template <class V>
hipError_t sub_register_semirings() {
    hipError_t e = sub_register<V, SR_MIN_PLUS>();
    if (e == hipSuccess) e = sub_register<V, SR_MAX_PLUS>();
    if (e == hipSuccess) e = sub_register<V, SR_MAX_MIN>();
    return e;
}

template <class V, int SR>
void issue_sub_pass(const ValLaunch& l, int pass, const ValSubArgs<V>& a, const int* list, hipStream_t s) {
    if (pass == 1) back_issue<SubRule<V, SR, 1>>(l, a, list, s);
    else if (pass == 2) back_issue<SubRule<V, SR, 2>>(l, a, list, s);
    else if (pass == 3) back_issue<SubRule<V, SR, 3>>(l, a, list, s);
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
