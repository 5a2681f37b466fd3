// semiring_check.cpp -- the value-level part of the value kernels' policy (csrc/mhs_semiring.hpp) on the host: for
// each semiring and both value types the identity of add, add (reg) commutative and associative on a literal
// table that includes +-Inf, and mul on literals; the enum and the names.  Built by tests/test_semiring_host.py
// with -fsanitize=address,undefined; prints "semiring ok".
#include "../mh-spgemm_amd/csrc/mhs_semiring.hpp"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <limits>

using namespace mhs;

static int failures = 0;
#define CHECK(cond)                                                    \
    do {                                                               \
        if (!(cond)) {                                                 \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                \
        }                                                              \
    } while (0)

// The laws of add (reg) in S on the table: x + identity == x on either side, commutative, associative
template <class S, class V>
static void laws() {
    const V inf = std::numeric_limits<V>::infinity();
    const V table[] = {V(-1000), V(-2.5), V(-0.1), V(0), V(0.1), V(1), V(2.5), V(1000), inf, -inf};
    const V e = S::template identity<V>();
    for (V x : table) {
        CHECK(S::reg(x, e) == x && S::reg(e, x) == x);
        for (V y : table) {
            CHECK(S::reg(x, y) == S::reg(y, x));
            for (V z : table) CHECK(S::reg(S::reg(x, y), z) == S::reg(x, S::reg(y, z)));
        }
    }
}

template <class V>
static void values() {
    const V inf = std::numeric_limits<V>::infinity(), nan = std::numeric_limits<V>::quiet_NaN();
    using PT = SrValue<SR_PLUS_TIMES>;
    using MinP = SrValue<SR_MIN_PLUS>;
    using MaxP = SrValue<SR_MAX_PLUS>;
    using MaxM = SrValue<SR_MAX_MIN>;
    // (plus rounds, so it is associative only up to rounding: its identity alone)
    for (V x : {V(-2.5), V(0), V(0.1), inf, -inf}) CHECK(PT::reg(x, PT::identity<V>()) == x && PT::reg(PT::identity<V>(), x) == x);
    laws<MinP, V>();
    laws<MaxP, V>();
    laws<MaxM, V>();
    // the identities
    CHECK(PT::identity<V>() == V(0) && MinP::identity<V>() == inf && MaxP::identity<V>() == -inf && MaxM::identity<V>() == -inf);
    // mul on literals
    CHECK(PT::mul(V(3), V(-0.5)) == V(-1.5));
    CHECK(MinP::mul(V(3), V(-0.5)) == V(2.5) && MaxP::mul(V(3), V(-0.5)) == V(2.5));
    CHECK(MinP::mul(V(7), inf) == inf && MaxP::mul(V(7), -inf) == -inf && MinP::mul(-inf, -inf) == -inf);
    CHECK(std::isnan(MinP::mul(inf, -inf)) && std::isnan(MaxP::mul(-inf, inf)));
    CHECK(MaxM::mul(V(3), V(-0.5)) == V(-0.5) && MaxM::mul(V(-0.5), V(3)) == V(-0.5) && MaxM::mul(V(2), V(2)) == V(2));
    CHECK(MaxM::mul(V(7), inf) == V(7) && MaxM::mul(-inf, V(7)) == -inf && MaxM::mul(inf, inf) == inf);
    CHECK(std::isnan(MaxM::mul(nan, V(1))) && std::isnan(MaxM::mul(V(1), nan)));  // a NaN operand is a NaN product
    // reg on literals, and a NaN product beside a number: the number where the NaN arrives, as minNum / maxNum
    CHECK(PT::reg(V(1), V(2)) == V(3) && MinP::reg(V(1), V(2)) == V(1) && MaxP::reg(V(1), V(2)) == V(2) && MaxM::reg(V(-1), V(-2)) == V(-1));
    CHECK(MinP::reg(V(1), nan) == V(1) && MaxP::reg(V(1), nan) == V(1) && MaxM::reg(V(1), nan) == V(1));
    CHECK(MinP::reg(inf, V(5)) == V(5) && MaxP::reg(-inf, V(-5)) == V(-5) && MinP::reg(inf, inf) == inf);
    // one relaxation step on literals: min(4 + 1, 2 + 2, Inf + 0) and its kin
    CHECK(MinP::reg(MinP::reg(MinP::reg(MinP::identity<V>(), MinP::mul(V(4), V(1))), MinP::mul(V(2), V(2))), MinP::mul(inf, V(0))) == V(4));
    CHECK(MaxP::reg(MaxP::reg(MaxP::identity<V>(), MaxP::mul(V(4), V(1))), MaxP::mul(V(2), V(2))) == V(5));
    CHECK(MaxM::reg(MaxM::reg(MaxM::identity<V>(), MaxM::mul(V(4), V(1))), MaxM::mul(V(2), V(3))) == V(2));
    // or-and on {0, 1}
    for (int a : {0, 1})
        for (int b : {0, 1})
            for (int c : {0, 1})
                for (int d : {0, 1})
                    CHECK(MaxM::reg(MaxM::reg(MaxM::identity<V>(), MaxM::mul(V(a), V(b))), MaxM::mul(V(c), V(d))) == V((a && b) || (c && d)));
}

int main() {
    CHECK(SR_PLUS_TIMES == 0 && SR_MIN_PLUS == 1 && SR_MAX_PLUS == 2 && SR_MAX_MIN == 3 && SR_COUNT == 4);
    CHECK(SrValue<SR_PLUS_TIMES>::id == 0 && SrValue<SR_MIN_PLUS>::id == 1 && SrValue<SR_MAX_PLUS>::id == 2 && SrValue<SR_MAX_MIN>::id == 3);
    for (int s : {-1, 4, 100}) CHECK(!val_semiring_ok(s) && !std::strcmp(val_semiring_name(s), "?"));
    const char* names[4] = {"plus_times", "min_plus", "max_plus", "max_min"};
    for (int s = 0; s < 4; ++s) CHECK(val_semiring_ok(s) && !std::strcmp(val_semiring_name(s), names[s]));
    values<double>();
    values<float>();
    if (failures) return 1;
    std::printf("semiring ok\n");
    return 0;
}
