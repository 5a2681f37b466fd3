// subgrad_check.cpp -- the value-level rule of the semiring subgradient (csrc/mhs_semiring.hpp: wins, share_a,
// share_b) on the host, for the three semirings and both value types: who wins, the identity and NaN exclusions, how
// mul's weight splits (the half split at a == b under max-min), +0 and -0 comparing equal, and the rule run as a
// sequential loop on a literal row -- ties, the even split and the gradient mass.  Built by
// tests/test_subgrad_host.py with -fsanitize=address,undefined; prints "subgrad ok".
#include "../mh-spgemm_amd/csrc/mhs_semiring.hpp"

#include <cmath>
#include <cstdio>
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

// One C entry reduced from the products of a[k] and b[k], then the rule as the kernels apply it: pass 1 counts the
// winners, pass 2 hands G / ties on.  Returns ties; dA and dB per product.
template <class S, class V>
static int entry(const std::vector<V>& a, const std::vector<V>& b, V G, std::vector<V>& dA, std::vector<V>& dB, V* cout = nullptr) {
    V c = S::template identity<V>();
    for (size_t k = 0; k < a.size(); ++k) c = S::reg(c, S::mul(a[k], b[k]));
    if (cout) *cout = c;
    int ties = 0;
    for (size_t k = 0; k < a.size(); ++k) ties += S::wins(a[k], b[k], c) ? 1 : 0;
    dA.assign(a.size(), V(0));
    dB.assign(a.size(), V(0));
    for (size_t k = 0; k < a.size(); ++k)
        if (S::wins(a[k], b[k], c)) {
            const V w = G / V(ties);
            dA[k] += S::share_a(a[k], b[k], w);
            dB[k] += S::share_b(a[k], b[k], w);
        }
    return ties;
}

template <class V>
static void rule() {
    const V inf = std::numeric_limits<V>::infinity(), nan = std::numeric_limits<V>::quiet_NaN();
    using MinP = SrValue<SR_MIN_PLUS>;
    using MaxP = SrValue<SR_MAX_PLUS>;
    using MaxM = SrValue<SR_MAX_MIN>;
    // winners: the product equals the entry
    CHECK(MinP::wins(V(1), V(2), V(3)) && !MinP::wins(V(1), V(2), V(2.5)) && !MinP::wins(V(1), V(2), V(4)));
    CHECK(MaxP::wins(V(-1), V(2), V(1)) && !MaxP::wins(V(-1), V(2), V(2)));
    CHECK(MaxM::wins(V(1), V(2), V(1)) && MaxM::wins(V(2), V(1), V(1)) && !MaxM::wins(V(1), V(2), V(2)));
    // (the one rounding of a + b is the forward's: 0.1 + 0.2 wins the entry it made and not its decimal neighbour)
    CHECK(MinP::wins(V(0.1), V(0.2), V(0.1) + V(0.2)));
    // an infinite entry that is not the identity has winners: -Inf under min-plus, +Inf under the max semirings
    CHECK(MinP::wins(-inf, V(1), -inf) && MaxP::wins(inf, V(1), inf) && MaxM::wins(inf, inf, inf));
    // the identity has none: an unreached entry, and "no path"
    CHECK(!MinP::wins(inf, V(1), inf) && !MinP::wins(inf, inf, inf) && !MinP::wins(V(1), V(2), inf));
    CHECK(!MaxP::wins(-inf, V(1), -inf) && !MaxP::wins(-inf, -inf, -inf));
    CHECK(!MaxM::wins(-inf, V(1), -inf) && !MaxM::wins(V(1), -inf, -inf) && !MaxM::wins(-inf, -inf, -inf));
    // a NaN never wins, on either side of the comparison
    CHECK(!MinP::wins(nan, V(1), V(1)) && !MinP::wins(V(1), nan, V(1)) && !MinP::wins(V(1), V(2), nan) && !MinP::wins(nan, V(1), nan));
    CHECK(!MinP::wins(inf, -inf, inf) && !MinP::wins(inf, -inf, -inf) && !MaxP::wins(-inf, inf, inf));  // Inf - Inf
    CHECK(!MaxP::wins(nan, V(1), V(1)) && !MaxP::wins(V(1), V(2), nan));
    CHECK(!MaxM::wins(nan, V(1), V(1)) && !MaxM::wins(V(1), nan, V(1)) && !MaxM::wins(V(1), V(2), nan) && !MaxM::wins(nan, nan, nan));
    // +0 and -0 compare equal
    const V pz = V(0), nz = -V(0);
    CHECK(std::signbit(nz) && !std::signbit(pz));
    CHECK(MinP::wins(V(1), V(-1), nz) && MinP::wins(nz, nz, pz) && MaxP::wins(pz, pz, nz));
    CHECK(MaxM::wins(pz, V(1), nz) && MaxM::wins(nz, V(1), pz) && MaxM::wins(nz, pz, nz));
    CHECK(MaxM::share_a(nz, pz, V(3)) == V(1.5) && MaxM::share_b(nz, pz, V(3)) == V(1.5));  // (equal operands: the half split)
    // the gradient of mul: all of w to both under the _plus semirings
    CHECK(MinP::share_a(V(1), V(2), V(0.75)) == V(0.75) && MinP::share_b(V(1), V(2), V(0.75)) == V(0.75));
    CHECK(MaxP::share_a(V(5), V(5), V(-3)) == V(-3) && MaxP::share_b(V(5), V(5), V(-3)) == V(-3));
    // ... under max-min to the smaller operand, half each where they are equal
    CHECK(MaxM::share_a(V(1), V(2), V(3)) == V(3) && MaxM::share_b(V(1), V(2), V(3)) == V(0));
    CHECK(MaxM::share_a(V(2), V(1), V(3)) == V(0) && MaxM::share_b(V(2), V(1), V(3)) == V(3));
    CHECK(MaxM::share_a(V(2), V(2), V(3)) == V(1.5) && MaxM::share_b(V(2), V(2), V(3)) == V(1.5));
    CHECK(MaxM::share_a(inf, inf, V(1)) == V(0.5) && MaxM::share_b(inf, inf, V(1)) == V(0.5));
    CHECK(MaxM::share_a(V(1), inf, V(4)) == V(4) && MaxM::share_b(V(1), inf, V(4)) == V(0));
    for (V w : {V(-2), V(0), V(0.5), V(7)})
        for (V a : {V(-1), V(0), V(2), inf})
            for (V b : {V(-1), V(0), V(2), inf}) CHECK(MaxM::share_a(a, b, w) + MaxM::share_b(a, b, w) == w);  // nothing is lost

    std::vector<V> dA, dB;
    V c;
    // min-plus: 1 + 3, 2 + 2, 5 + 0 and 4 + 0 -- three winners of 4 share G = 6
    CHECK((entry<MinP, V>({1, 2, 5, 4}, {3, 2, 0, 0}, V(6), dA, dB, &c)) == 3 && c == V(4));
    CHECK(dA[0] == V(2) && dA[1] == V(2) && dA[2] == V(0) && dA[3] == V(2) && dB[0] == V(2) && dB[2] == V(0) && dB[3] == V(2));
    // max-plus on the same products: one winner
    CHECK((entry<MaxP, V>({1, 2, 5, 4}, {3, 2, 0, 0}, V(6), dA, dB, &c)) == 1 && c == V(5));
    CHECK(dA[2] == V(6) && dB[2] == V(6) && dA[0] == V(0) && dB[3] == V(0));
    // a NaN product beside a number: the number wins alone (reg keeps it), the NaN product gets nothing
    CHECK((entry<MinP, V>({1, nan}, {3, 0}, V(2), dA, dB, &c)) == 1 && c == V(4) && dA[0] == V(2) && dA[1] == V(0) && dB[1] == V(0));
    // no path: every product +Inf under min-plus passes nothing
    CHECK((entry<MinP, V>({inf, 1}, {0, inf}, V(2), dA, dB, &c)) == 0 && c == inf && dA[0] == V(0) && dA[1] == V(0) && dB[0] == V(0));
    // an unreached entry
    CHECK((entry<MaxM, V>({}, {}, V(2), dA, dB, &c)) == 0 && c == -inf);
    // max-min on {0, 1}: or-and, where ties are the rule -- min(1,1), min(1,0), min(1,1), min(0,0); two winners of 1,
    // each split between its equal operands; the mass is G
    CHECK((entry<MaxM, V>({1, 1, 1, 0}, {1, 0, 1, 0}, V(8), dA, dB, &c)) == 2 && c == V(1));
    CHECK(dA[0] == V(2) && dB[0] == V(2) && dA[2] == V(2) && dB[2] == V(2) && dA[1] == V(0) && dB[1] == V(0) && dA[3] == V(0));
    V mass = 0;
    for (size_t k = 0; k < dA.size(); ++k) mass += dA[k] + dB[k];
    CHECK(mass == V(8));
    // max-min with unequal operands: min(3, 5) and min(7, 3) tie at 3; A gets the first's weight, B the second's
    CHECK((entry<MaxM, V>({3, 7, 1}, {5, 3, 9}, V(4), dA, dB, &c)) == 2 && c == V(3));
    CHECK(dA[0] == V(2) && dB[0] == V(0) && dA[1] == V(0) && dB[1] == V(2) && dA[2] == V(0) && dB[2] == V(0));
}

int main() {
    rule<double>();
    rule<float>();
    if (failures) return 1;
    std::printf("subgrad ok\n");
    return 0;
}
