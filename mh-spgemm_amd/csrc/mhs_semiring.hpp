// mhs_semiring.hpp -- the algebra of a values plan (mhs_values_plan_create_semiring), as values.
//
// A values plan has a fourth fixed property beside its value type, its width and its mask form: the semiring
// (add, mul, the identity of add) its kernels reduce the kept products with.
//
//   semiring        add   mul   identity of add
//   SR_PLUS_TIMES   +     x     0                 every plan of the other creation calls
//   SR_MIN_PLUS     min   +     +Inf              one relaxation step of shortest paths
//   SR_MAX_PLUS     max   +     -Inf              longest / critical paths, Viterbi-style scoring
//   SR_MAX_MIN      max   min   -Inf              widest (bottleneck) paths; on {0, 1} the boolean or-and product
//
// SrValue<SR> is the value-level part of a kernel's policy: identity(), mul(a, b) and reg(x, v), the register
// reduce of the dot class.  The memory-level part -- the LDS and the global atomic of a class's reduce -- is
// SrPolicy<SR> of mhs_valwalk.hpp, which derives from it.  min and max are exact and do not depend on order, and the
// one rounding of a + b does not either: a result of the three new semirings has the bits of any sequential
// evaluation (the sign of a zero apart).  A NaN product is not ordered: reg() keeps the other side where it can, as
// the hardware atomics (minNum / maxNum) do, so such an entry is NaN or the reduce of its other products.  The mul of
// SR_MAX_MIN hands a NaN operand on, so that a NaN operand makes a NaN product under every semiring.
// The three new semirings also carry the value-level rule of their subgradient (mhs_spgemm_values_subgrad; the rule is
// in include/mhspgemm.h): wins(a, b, c) -- whether the product of a and b is a winner of an entry whose forward result
// is c: mul(a, b) == c as values (so +0 == -0, and a NaN on either side is no winner) and c is not the identity of add
// -- and share_a(a, b, w) / share_b(a, b, w), what of a winner's weight w goes to the A entry and to the B entry: all
// of it to both under the _PLUS semirings, under max-min to the smaller operand, half to each where they are equal.
// No pointer and no HIP type in here: tests/semiring_check.cpp and tests/subgrad_check.cpp run it on the host.
#pragma once
#include <limits>

namespace mhs {

enum ValSemiring : int { SR_PLUS_TIMES = 0, SR_MIN_PLUS = 1, SR_MAX_PLUS = 2, SR_MAX_MIN = 3, SR_COUNT = 4 };

constexpr bool val_semiring_ok(int sr) { return sr >= SR_PLUS_TIMES && sr < SR_COUNT; }
// (the names of the Python mirror's SEMIRINGS and of the CLI's --semiring)
constexpr const char* val_semiring_name(int sr) {
    return sr == SR_PLUS_TIMES ? "plus_times" : sr == SR_MIN_PLUS ? "min_plus" : sr == SR_MAX_PLUS ? "max_plus"
           : sr == SR_MAX_MIN  ? "max_min"    : "?";
}

// The smaller / the larger of two values; of a NaN and a number, the number when the NaN is v, x's own NaN otherwise
template <class V>
constexpr V sr_min(V x, V v) { return v < x ? v : x; }
template <class V>
constexpr V sr_max(V x, V v) { return v > x ? v : x; }

template <int SR>
struct SrValue;
template <>
struct SrValue<SR_PLUS_TIMES> {
    static constexpr int id = SR_PLUS_TIMES;
    template <class V> static constexpr V identity() { return V(0); }
    template <class V> static constexpr V mul(V a, V b) { return a * b; }
    template <class V> static constexpr V reg(V x, V v) { return x + v; }
};
template <>
struct SrValue<SR_MIN_PLUS> {
    static constexpr int id = SR_MIN_PLUS;
    template <class V> static constexpr V identity() { return std::numeric_limits<V>::infinity(); }
    template <class V> static constexpr V mul(V a, V b) { return a + b; }
    template <class V> static constexpr V reg(V x, V v) { return sr_min(x, v); }
    template <class V> static constexpr bool wins(V a, V b, V c) { return mul(a, b) == c && c != identity<V>(); }
    template <class V> static constexpr V share_a(V, V, V w) { return w; }
    template <class V> static constexpr V share_b(V, V, V w) { return w; }
};
template <>
struct SrValue<SR_MAX_PLUS> {
    static constexpr int id = SR_MAX_PLUS;
    template <class V> static constexpr V identity() { return -std::numeric_limits<V>::infinity(); }
    template <class V> static constexpr V mul(V a, V b) { return a + b; }
    template <class V> static constexpr V reg(V x, V v) { return sr_max(x, v); }
    template <class V> static constexpr bool wins(V a, V b, V c) { return mul(a, b) == c && c != identity<V>(); }
    template <class V> static constexpr V share_a(V, V, V w) { return w; }
    template <class V> static constexpr V share_b(V, V, V w) { return w; }
};
template <>
struct SrValue<SR_MAX_MIN> {
    static constexpr int id = SR_MAX_MIN;
    template <class V> static constexpr V identity() { return -std::numeric_limits<V>::infinity(); }
    // min(a, b) that hands a NaN of either side on
    template <class V> static constexpr V mul(V a, V b) { return (a < b || a != a) ? a : b; }
    template <class V> static constexpr V reg(V x, V v) { return sr_max(x, v); }
    template <class V> static constexpr bool wins(V a, V b, V c) { return mul(a, b) == c && c != identity<V>(); }
    template <class V> static constexpr V share_a(V a, V b, V w) { return a < b ? w : a == b ? w / V(2) : V(0); }
    template <class V> static constexpr V share_b(V a, V b, V w) { return b < a ? w : a == b ? w / V(2) : V(0); }
};

}  // namespace mhs
