// smooth_check.cpp -- the value-level part of the smoothed value kernels (csrc/mhs_smooth.hpp) on the host, on
// literals and for both value types: the identity guards, +-Inf, NaN, min-plus as the negation of max-plus,
// finish(M, 1) == M, the weight's zeros and ones, and the global class's logaddexp against term / finish.
// Built by tests/test_smooth_host.py with -fsanitize=address,undefined; prints "smooth ok".
#include "../mh-spgemm_amd/csrc/mhs_smooth.hpp"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <limits>
#include <vector>

using namespace mhs;

static int failures = 0;
#define CHECK(cond)                                                    \
    do {                                                               \
        if (!(cond)) {                                                 \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                \
        }                                                              \
    } while (0)

// The LDS classes' scheme, sequentially: the signed products, their max, the sum of their terms, the finish, the sign
template <class V>
static V forward(int sr, const std::vector<V>& a, const std::vector<V>& b) {
    using S = Smooth<V>;
    const V sg = V(val_smooth_sign(sr));
    V M = S::floor(), s = V(0);
    for (size_t k = 0; k < a.size(); ++k) M = S::max(M, S::mul(sg, a[k], b[k]));
    for (size_t k = 0; k < a.size(); ++k) s += S::term(S::mul(sg, a[k], b[k]), M);
    return sg * S::finish(M, s);
}
// The global class's: the running result updated by one product after another
template <class V>
static V forward_global(int sr, const std::vector<V>& a, const std::vector<V>& b) {
    using S = Smooth<V>;
    const V sg = V(val_smooth_sign(sr));
    V c = sg * S::floor();
    for (size_t k = 0; k < a.size(); ++k) c = sg * S::logaddexp(sg * c, S::mul(sg, a[k], b[k]));
    return c;
}

template <class V>
static void values() {
    using S = Smooth<V>;
    const V inf = std::numeric_limits<V>::infinity(), nan = std::numeric_limits<V>::quiet_NaN();
    const V eps = std::numeric_limits<V>::epsilon();
    const V ln2 = V(0.6931471805599453L);
    // the signed product: one add, an exact sign
    CHECK(S::mul(V(1), V(3), V(-0.5)) == V(2.5) && S::mul(V(-1), V(3), V(-0.5)) == V(-2.5));
    CHECK(S::mul(V(-1), V(7), inf) == -inf && S::mul(V(1), V(7), -inf) == -inf && std::isnan(S::mul(V(1), inf, -inf)));
    CHECK(S::floor() == -inf && S::finite(V(0)) && S::finite(V(-1e30)) && !S::finite(inf) && !S::finite(-inf) && !S::finite(nan));
    CHECK(S::max(V(1), V(2)) == V(2) && S::max(V(2), V(1)) == V(2) && S::max(V(1), nan) == V(1) && S::max(-inf, V(-5)) == V(-5));
    // term: 1 at the max, 0 where the max is not finite (v - M would be NaN), a NaN product stays
    CHECK(S::term(V(3), V(3)) == V(1) && S::term(V(-1000), V(-1000)) == V(1));
    CHECK(S::term(-inf, -inf) == V(0) && S::term(inf, inf) == V(0) && S::term(V(5), inf) == V(0) && S::term(-inf, V(5)) == V(0));
    CHECK(std::isnan(S::term(nan, V(1))) && std::isnan(S::term(nan, -inf)) && std::isnan(S::term(nan, inf)));
    CHECK(std::fabs(S::term(V(2), V(3)) - V(0.36787944117144233L)) <= 2 * eps);
    CHECK(S::term(V(-2048), V(0)) == V(0));  // (the wide gaps of the exact anchors underflow to exactly 0)
    // finish: M where the sum is 1 and where M is not finite; a NaN sum stays
    for (V M : {V(-1000), V(-2.5), V(0), V(0.1), V(1e6)}) CHECK(S::finish(M, V(1)) == M);
    CHECK(S::finish(-inf, V(0)) == -inf && S::finish(inf, V(0)) == inf && S::finish(inf, V(3)) == inf);
    CHECK(std::isnan(S::finish(V(1), nan)) && std::isnan(S::finish(-inf, nan)) && std::isnan(S::finish(inf, nan)));
    CHECK(std::fabs(S::finish(V(5), V(2)) - (V(5) + ln2)) <= 8 * eps);
    // weight: 0 for a result that is not finite, 1 * g where the product is the result
    for (V c : {inf, -inf, nan})
        for (V v : {V(0), V(3), inf, -inf, nan}) CHECK(S::weight(v, c, V(7)) == V(0) && !std::signbit(S::weight(v, c, V(7))));
    for (V g : {V(-3), V(0), V(0.25), V(1e10)}) CHECK(S::weight(V(2.5), V(2.5), g) == g);
    CHECK(S::weight(-inf, V(0), V(5)) == V(0));  // an identity product beside finite ones
    CHECK(std::fabs(S::weight(V(1), V(1) + ln2, V(4)) - V(2)) <= 8 * eps);
    // logaddexp: the identity on either side, the opposite infinity, NaN
    CHECK(S::logaddexp(-inf, V(3)) == V(3) && S::logaddexp(V(3), -inf) == V(3) && S::logaddexp(-inf, -inf) == -inf);
    CHECK(S::logaddexp(inf, V(3)) == inf && S::logaddexp(V(3), inf) == inf && S::logaddexp(inf, inf) == inf && S::logaddexp(inf, -inf) == inf);
    CHECK(std::isnan(S::logaddexp(nan, V(1))) && std::isnan(S::logaddexp(V(1), nan)) && std::isnan(S::logaddexp(-inf, nan)));
    CHECK(std::fabs(S::logaddexp(V(2), V(2)) - (V(2) + ln2)) <= 8 * eps && S::logaddexp(V(0), V(-4096)) == V(0));

    for (int sr : {SR_MIN_PLUS, SR_MAX_PLUS}) {
        const V id = sr == SR_MIN_PLUS ? inf : -inf, opp = -id;
        for (auto fwd : {forward<V>, forward_global<V>}) {
            CHECK(fwd(sr, {}, {}) == id);                                           // no product
            CHECK(fwd(sr, {V(1), V(2)}, {id, id}) == id);                           // "no edge" everywhere
            CHECK(fwd(sr, {V(1.5)}, {V(2)}) == V(3.5));                             // one product: its bits
            CHECK(fwd(sr, {V(1.5), V(7)}, {V(2), id}) == V(3.5));                   // an identity product is ignored
            CHECK(fwd(sr, {V(1.5), V(7)}, {V(2), opp}) == opp);                     // the opposite infinity
            CHECK(std::isnan(fwd(sr, {V(1.5), nan}, {V(2), V(1)})));                // a NaN operand
            CHECK(std::isnan(fwd(sr, {inf}, {-inf})));                              // +Inf + -Inf
        }
        // two equal products: log 2 apart from the hard reduce, on the soft side of it
        const V two = forward<V>(sr, {V(1), V(2)}, {V(2), V(1)});
        CHECK(std::fabs(two - (sr == SR_MIN_PLUS ? V(3) - ln2 : V(3) + ln2)) <= 8 * eps);
        CHECK(std::fabs(forward_global<V>(sr, {V(1), V(2)}, {V(2), V(1)}) - two) <= 8 * eps);
    }
    // min-plus is the negation of max-plus on negated operands, bit for bit
    const std::vector<V> a = {V(0.3), V(-7.25), V(4), V(1.5), V(-0.125)}, b = {V(2.5), V(6.5), V(-3.75), V(0.7), V(0.9)};
    std::vector<V> na(a), nb(b);
    for (V& x : na) x = -x;
    for (V& x : nb) x = -x;
    CHECK(forward<V>(SR_MIN_PLUS, a, b) == -forward<V>(SR_MAX_PLUS, na, nb));
    CHECK(forward_global<V>(SR_MIN_PLUS, a, b) == -forward_global<V>(SR_MAX_PLUS, na, nb));
    CHECK(std::fabs(forward<V>(SR_MAX_PLUS, a, b) - forward_global<V>(SR_MAX_PLUS, a, b)) <= 16 * eps);
    // the weights of an entry sum to its cotangent (softmax weights)
    const V c = forward<V>(SR_MAX_PLUS, a, b);
    V mass = V(0);
    for (size_t k = 0; k < a.size(); ++k) mass += S::weight(S::mul(V(1), a[k], b[k]), c, V(3));
    CHECK(std::fabs(mass - V(3)) <= 32 * eps);
}

int main() {
    CHECK(SMOOTH_NONE == 0 && SMOOTH_LSE == 1 && val_smooth_ok(0) && val_smooth_ok(1) && !val_smooth_ok(-1) && !val_smooth_ok(2));
    CHECK(val_smooth_serves(SR_MIN_PLUS) && val_smooth_serves(SR_MAX_PLUS) && !val_smooth_serves(SR_PLUS_TIMES) &&
          !val_smooth_serves(SR_MAX_MIN) && !val_smooth_serves(4) && !val_smooth_serves(-1));
    CHECK(val_smooth_sign(SR_MIN_PLUS) == -1 && val_smooth_sign(SR_MAX_PLUS) == 1);
    CHECK(val_smooth_planes(SMOOTH_NONE) == 1 && val_smooth_planes(SMOOTH_LSE) == 2);
    CHECK(!std::strcmp(val_smooth_name(0), "none") && !std::strcmp(val_smooth_name(1), "lse") && !std::strcmp(val_smooth_name(2), "?"));
    CHECK(SR_COUNT == 4);  // (smoothing is no semiring)
    values<double>();
    values<float>();
    if (failures) return 1;
    std::printf("smooth ok\n");
    return 0;
}
