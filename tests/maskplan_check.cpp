// maskplan_check.cpp -- the masked values plan's row rule and its launch (csrc/mhs_valplan.hpp) on the
// host: val_class_masked one below, at and one above VAL_DOT_RATIO x dot_cost == products in every
// form, rows without mask entries, A entries or products, the dot-cost arithmetic, and plan_values
// with and without dot rows.  Built by tests/test_masked_host.py with -fsanitize=address,undefined;
// prints "maskplan ok".
#include "../mh-spgemm_amd/csrc/mhs_valplan.hpp"

#include <cstdio>
#include <cstring>
#include <initializer_list>

using namespace mhs;

static int failures = 0;
#define CHECK(cond)                                                    \
    do {                                                               \
        if (!(cond)) {                                                 \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                \
        }                                                              \
    } while (0)

static ValCounts one(int cls, int rows, int need) {
    ValCounts c{};
    c.rows[cls] = rows;
    c.need[cls] = need;
    return c;
}

int main() {
    CHECK(VC_DOT == 7 && VC_COUNT == 7 && VAL_NCLASS == 8 && VAL_PLAN_MAX == 8);
    CHECK(VAL_DOT_RATIO >= 1 && VAL_DOT_RATIO <= 64);
    CHECK(VM_AUTO == 0 && VM_PRODUCT == 1 && VM_DOT == 2);

    // ---- the dot cost: 1 + ceil_log2(len + 1) steps per mask entry
    CHECK(val_ceil_log2(1) == 0 && val_ceil_log2(2) == 1 && val_ceil_log2(3) == 2 && val_ceil_log2(4) == 2 &&
          val_ceil_log2(5) == 3 && val_ceil_log2(64) == 6 && val_ceil_log2(65) == 7 && val_ceil_log2(601) == 10);
    CHECK(val_dot_steps(0) == 1 && val_dot_steps(1) == 2 && val_dot_steps(3) == 3 && val_dot_steps(64) == 8 &&
          val_dot_steps(600) == 11);
    CHECK(val_sat_add(5, 6) == 11 && val_sat_add(VAL_SAT - 1, 5) == VAL_SAT && val_sat_add(VAL_SAT, VAL_SAT) == VAL_SAT);
    CHECK(val_sat_mul(0, VAL_SAT) == 0 && val_sat_mul(3, 7) == 21 && val_sat_mul(1LL << 40, 1LL << 40) == VAL_SAT &&
          val_sat_mul(2, VAL_SAT / 2 + 1) == VAL_SAT);

    // ---- the rule at the threshold, in each form.  A row of 10 mask entries over 50 columns and 8 A entries
    // with dot_cost 160; `other` is what the product form gives it.
    const int n = 10, nA = 8;
    const long long span = 50, cost = 160;
    for (int ratio : {1, 2, 4, 8, 16, 32, 64, VAL_DOT_RATIO}) {
        const long long at = (long long)ratio * cost;
        for (long long products : {at - 1, at, at + 1}) {
            const int other = val_class(n, span, products);
            CHECK(other != VC_DOT);
            CHECK(val_class_masked(n, span, products, nA, cost, VM_PRODUCT, ratio) == other);
            CHECK(val_class_masked(n, span, products, nA, cost, VM_DOT, ratio) == VC_DOT);
            // AUTO: the dot class only when ratio x dot_cost < products
            CHECK(val_class_masked(n, span, products, nA, cost, VM_AUTO, ratio) == (products > at ? VC_DOT : other));
        }
    }
    // the default ratio is VAL_DOT_RATIO
    CHECK(val_class_masked(n, span, VAL_DOT_RATIO * cost + 1, nA, cost, VM_AUTO) == VC_DOT);
    CHECK(val_class_masked(n, span, VAL_DOT_RATIO * cost, nA, cost, VM_AUTO) == val_class(n, span, VAL_DOT_RATIO * cost));
    // a saturated cost never beats a product count
    CHECK(val_class_masked(n, 1000000, VAL_SAT, nA, VAL_SAT, VM_AUTO, 1) == VC_BLOCK_SEARCH);
    CHECK(val_class_masked(n, 1000000, VAL_SAT, nA, VAL_SAT / 2 + 1, VM_AUTO, 2) == VC_BLOCK_SEARCH);

    // ---- rows without mask entries, without A entries, without products: never the dot class
    for (int form : {VM_AUTO, VM_PRODUCT, VM_DOT}) {
        CHECK(val_class_masked(0, 0, 100000, 8, 0, form) == VC_NONE);      // n == 0 (dot_cost 0 < products)
        CHECK(val_class_masked(0, 0, 0, 0, 0, form) == VC_NONE);
        CHECK(val_class_masked(10, 50, 0, 0, 0, form) == VC_TEAM);         // nA == 0: the team zero-fills
        CHECK(val_class_masked(100, 500, 0, 0, 0, form) == VC_GLOBAL);     // ... or the global class
    }
    // products == 0 with A entries (every B row empty): zero either way; AUTO stays in product form
    CHECK(val_class_masked(10, 50, 0, 8, 160, VM_AUTO) == VC_TEAM);
    CHECK(val_class_masked(10, 50, 0, 8, 160, VM_PRODUCT) == VC_TEAM);
    CHECK(val_class_masked(10, 50, 0, 8, 160, VM_DOT) == VC_DOT);
    // the containing-mask case: n * nA >= products, and a step count is at least 1 per entry
    CHECK(val_class_masked(40, 4000, 320, 8, 8 * 40 * 1, VM_AUTO, 1) == val_class(40, 4000, 320));
    // the hub case of the GPU test: 2 mask entries, 8 A entries, B^T rows of 64: cost 128 against 32,768 products
    CHECK(8 * 2 * val_dot_steps(64) == 128);
    for (int ratio : {1, 2, 64}) CHECK(val_class_masked(2, 3000, 32768, 8, 128, VM_AUTO, ratio) == VC_DOT);
    // the dot class needs no LDS region
    CHECK(val_row_need(VC_DOT, 100, 100000) == 0 && val_class_cap(VC_DOT) == 0);

    // ---- plan_values with dot rows: exactly one VK_DOT launch more, 1 <= grid <= rows
    for (int rows : {1, 2, 3, 4, 5, 1000, 70000, 5000000}) {
        const ValPlan p = plan_values(one(VC_DOT, rows, 0));
        CHECK(p.n == 1 && p.launch[0].kernel == VK_DOT && p.launch[0].cls == VC_DOT && p.launch[0].count == rows);
        CHECK(p.launch[0].grid >= 1 && p.launch[0].grid <= rows && p.launch[0].grid <= 16384);
        CHECK(p.launch[0].grid == ((rows + 3) / 4 < 16384 ? (rows + 3) / 4 : 16384));
        CHECK(p.launch[0].block == 256 && p.launch[0].lds == 0 && p.launch[0].region == 0);
    }
    {   // every class at once (the counts of valplan_check.cpp): the six launches of today, in today's order ...
        ValCounts c{};
        for (int k = 0; k < VC_COUNT; ++k) {
            c.rows[k] = 10 * (k + 1);
            c.need[k] = val_class_cap(k);
        }
        const ValPlan p = plan_values(c);
        CHECK(p.n == 6);
        const int order[6] = {VC_GLOBAL, VC_BLOCK_SEARCH, VC_BLOCK_DIRECT, VC_WAVE_SEARCH, VC_WAVE_DIRECT, VC_TEAM};
        const int kern[6] = {VK_GLOBAL, VK_BLOCK_SEARCH, VK_BLOCK_DIRECT, VK_WAVE_SEARCH, VK_WAVE_DIRECT, VK_TEAM};
        const int grid[6] = {70, 60, 50, 10, 8, 1}, block[6] = {1024, 1024, 1024, 256, 256, 256};
        const int lds[6] = {0, 159744, 159744, 32768, 32768, 24576};
        for (int i = 0; i < 6 && i < p.n; ++i) {
            CHECK(p.launch[i].cls == order[i] && p.launch[i].kernel == kern[i] && p.launch[i].count == c.rows[order[i]]);
            CHECK(p.launch[i].grid == grid[i] && p.launch[i].block == block[i] && p.launch[i].lds == lds[i]);
            CHECK(p.launch[i].kernel != VK_DOT);
        }
        // ... and with dot rows the same six and one VK_DOT launch, nothing else changed
        ValCounts d = c;
        d.rows[VC_DOT] = 9;
        const ValPlan q = plan_values(d);
        CHECK(q.n == 7);
        int dots = 0, j = 0;
        for (int i = 0; i < q.n; ++i) {
            if (q.launch[i].kernel == VK_DOT) {
                ++dots;
                CHECK(q.launch[i].cls == VC_DOT && q.launch[i].count == 9 && q.launch[i].grid == 3);
                continue;
            }
            CHECK(j < 6 && std::memcmp(&q.launch[i], &p.launch[j], sizeof(ValLaunch)) == 0);
            ++j;
        }
        CHECK(dots == 1 && j == 6);
    }

    if (failures) return 1;
    std::printf("maskplan ok\n");
    return 0;
}
