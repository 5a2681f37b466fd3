// mhs_smooth.hpp -- the smoothing of a values plan (mhs_values_plan_create_smooth), as values.
//
// A values plan has a sixth fixed property beside its value type, width, mask form, semiring and sum type: whether its
// reduce is smoothed.  SMOOTH_LSE on a min-plus or max-plus plan replaces the hard min / max by log-sum-exp at unit
// temperature:
//   max-plus   C = log sum_k exp(v_k)          v_k = fl(A(i,k) + B(k,j)), formed once in the plan's type
//   min-plus   C = -log sum_k exp(-v_k)
// Negation is exact, so there is one policy: the kernels work on the signed products sg * v_k (sg = +1 under max-plus,
// -1 under min-plus), reduce them as under max-plus, and hand sg * result out.  In that signed domain the identity of
// the hard reduce is -Inf ("no edge") and the opposite infinity is +Inf.
//
// Smooth<V> is the value-level part of the smoothed kernels (mhs_values_smooth.hip):
//   mul(sg, a, b)    the signed product sg * (a + b): the one rounding of the add
//   floor()          -Inf: what the max plane of an entry starts from
//   term(v, M)       what a product adds to its entry's sum once the entry's max M is known: exp(v - M), exactly 1 where
//                    v == M; 0 where M is not finite (v - M would be NaN there, and finish() hands such an M on); a NaN
//                    product stays NaN
//   finish(M, s)     the entry from its max and its sum: M + log(s); M itself where s == 1 (one product: its bits) and
//                    where M is not finite -- -Inf: no product, or every product "no edge"; +Inf: a product equal to
//                    the opposite infinity --; a NaN sum stays NaN
//   logaddexp(c, v)  the global class's update of a running result c by a product v, with the same guards:
//                    max + log1p(exp(-|c - v|))
//   weight(v, c, g)  the gradient's weight of a product v of an entry whose (signed) forward result is c and whose
//                    cotangent is g: g * exp(v - c), exactly g where v == c, exactly 0 where c is not finite
// and of their reference on the host.  No pointer and no HIP type in here: tests/smooth_check.cpp runs it on the host.
#pragma once
#include "mhs_semiring.hpp"

#include <cmath>
#include <limits>

#ifdef __HIPCC__
#define MHS_SMOOTH_FN __host__ __device__ inline
#else
#define MHS_SMOOTH_FN inline
#endif

namespace mhs {

enum ValSmooth : int { SMOOTH_NONE = 0, SMOOTH_LSE = 1 };

constexpr bool val_smooth_ok(int smooth) { return smooth == SMOOTH_NONE || smooth == SMOOTH_LSE; }
// the semirings that have a smoothed reduce
constexpr bool val_smooth_serves(int sr) { return sr == SR_MIN_PLUS || sr == SR_MAX_PLUS; }
// (the names of the Python mirror's smooth= and of the CLI's --smooth)
constexpr const char* val_smooth_name(int smooth) { return smooth == SMOOTH_NONE ? "none" : smooth == SMOOTH_LSE ? "lse" : "?"; }
// the sign the products of a smoothed plan are taken with
constexpr int val_smooth_sign(int sr) { return sr == SR_MIN_PLUS ? -1 : 1; }
// A smoothed plan holds two planes per C entry, a running max and a sum: it classifies at twice the sum bytes
constexpr int val_smooth_planes(int smooth) { return smooth == SMOOTH_LSE ? 2 : 1; }

template <class V>
struct Smooth {
    static constexpr V inf() { return std::numeric_limits<V>::infinity(); }
    static constexpr V floor() { return -inf(); }
    static constexpr bool finite(V x) { return x > -inf() && x < inf(); }  // (false for a NaN)
    static constexpr V mul(V sg, V a, V b) { return sg * (a + b); }
    static constexpr V max(V x, V v) { return sr_max(x, v); }  // (a NaN product is skipped, as the hardware's maxNum does)
    static MHS_SMOOTH_FN V term(V v, V M) {
        if (v != v) return v;
        if (!finite(M)) return V(0);
        return v == M ? V(1) : std::exp(v - M);
    }
    static MHS_SMOOTH_FN V finish(V M, V s) {
        if (s != s) return s;
        if (!finite(M) || s == V(1)) return M;
        return M + std::log(s);
    }
    static MHS_SMOOTH_FN V logaddexp(V c, V v) {
        if (v != v) return v;
        if (c != c) return c;
        if (v == -inf()) return c;
        if (c == -inf()) return v;
        if (c == inf() || v == inf()) return inf();
        const V d = c - v;
        return (d > V(0) ? c : v) + std::log1p(std::exp(d > V(0) ? -d : d));
    }
    static MHS_SMOOTH_FN V weight(V v, V c, V g) {
        if (!finite(c)) return V(0);
        return v == c ? g : g * std::exp(v - c);
    }
};

}  // namespace mhs
