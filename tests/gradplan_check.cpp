// gradplan_check.cpp -- the launch plan of the values backward (plan_grad, csrc/mhs_valplan.hpp) on the
// host: the forward's launches of the product-form classes, unchanged, and a masked plan's dot rows routed
// to the global-form kernel a wave per row.  Built by tests/test_values_grad_host.py with
// -fsanitize=address,undefined; prints "gradplan ok".
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

int main() {
    // ---- no rows: no launch
    CHECK(plan_grad(ValCounts{}).n == 0);

    // ---- every product-form class at once: the launches of plan_values, field by field, against literals
    ValCounts c{};
    for (int k = 0; k < VC_COUNT; ++k) {
        c.rows[k] = 10 * (k + 1);
        c.need[k] = val_class_cap(k);
    }
    const ValPlan p = plan_grad(c);
    const ValPlan f = plan_values(c);
    CHECK(p.n == 6 && f.n == 6);
    const int order[6] = {VC_GLOBAL, VC_BLOCK_SEARCH, VC_BLOCK_DIRECT, VC_WAVE_SEARCH, VC_WAVE_DIRECT, VC_TEAM};
    const int kern[6] = {VK_GLOBAL, VK_BLOCK_SEARCH, VK_BLOCK_DIRECT, VK_WAVE_SEARCH, VK_WAVE_DIRECT, VK_TEAM};
    const int grid[6] = {70, 60, 50, 10, 8, 1}, block[6] = {1024, 1024, 1024, 256, 256, 256};
    const int lds[6] = {0, 159744, 159744, 32768, 32768, 24576};
    const int region[6] = {0, 159744, 159744, 8192, 8192, 768};
    for (int i = 0; i < 6 && i < p.n; ++i) {
        CHECK(p.launch[i].cls == order[i] && p.launch[i].kernel == kern[i] && p.launch[i].count == c.rows[order[i]]);
        CHECK(p.launch[i].grid == grid[i] && p.launch[i].block == block[i] && p.launch[i].lds == lds[i]);
        CHECK(p.launch[i].region == region[i]);
        CHECK(std::memcmp(&p.launch[i], &f.launch[i], sizeof(ValLaunch)) == 0);
    }
    // small needs: the 256-thread block launches and the declared (not the capped) LDS
    {
        ValCounts s{};
        s.rows[VC_BLOCK_DIRECT] = 5000, s.need[VC_BLOCK_DIRECT] = 30000;
        s.rows[VC_WAVE_SEARCH] = 9, s.need[VC_WAVE_SEARCH] = 1000;
        s.rows[VC_TEAM] = 33, s.need[VC_TEAM] = 100;
        const ValPlan q = plan_grad(s);
        CHECK(q.n == 3);
        CHECK(q.launch[0].kernel == VK_BLOCK_DIRECT && q.launch[0].grid == 4096 && q.launch[0].block == 256 &&
              q.launch[0].lds == 30720 && q.launch[0].region == 30720 && q.launch[0].count == 5000);
        CHECK(q.launch[1].kernel == VK_WAVE_SEARCH && q.launch[1].grid == 3 && q.launch[1].block == 256 &&
              q.launch[1].lds == 4096 && q.launch[1].region == 1024 && q.launch[1].count == 9);
        CHECK(q.launch[2].kernel == VK_TEAM && q.launch[2].grid == 2 && q.launch[2].block == 256 && q.launch[2].lds == 32 * 120 &&
              q.launch[2].region == 120 && q.launch[2].count == 33);
    }

    // ---- dot rows: the global-form kernel on the dot list, a wave per row; never VK_DOT
    for (int rows : {1, 2, 3, 4, 5, 1000, 70000, 5000000}) {
        ValCounts d{};
        d.rows[VC_DOT] = rows;
        const ValPlan q = plan_grad(d);
        CHECK(q.n == 1 && q.launch[0].kernel == VK_GLOBAL && q.launch[0].cls == VC_DOT && q.launch[0].count == rows);
        CHECK(q.launch[0].grid == ((rows + 3) / 4 < 16384 ? (rows + 3) / 4 : 16384));
        CHECK(q.launch[0].block == 256 && q.launch[0].lds == 0 && q.launch[0].region == 0);
    }
    {   // with the six others: seven launches, two of the global-form kernel told apart by their block size
        ValCounts d = c;
        d.rows[VC_DOT] = 9;
        const ValPlan q = plan_grad(d);
        CHECK(q.n == 7);
        int globals = 0, j = 0;
        for (int i = 0; i < q.n; ++i) {
            CHECK(q.launch[i].kernel != VK_DOT);
            if (q.launch[i].cls == VC_DOT) {
                CHECK(q.launch[i].kernel == VK_GLOBAL && q.launch[i].block == 256 && q.launch[i].count == 9 && q.launch[i].grid == 3);
                ++globals;
                continue;
            }
            if (q.launch[i].kernel == VK_GLOBAL) {
                CHECK(q.launch[i].cls == VC_GLOBAL && q.launch[i].block == 1024);
                ++globals;
            }
            CHECK(j < 6 && std::memcmp(&q.launch[i], &p.launch[j], sizeof(ValLaunch)) == 0);
            ++j;
        }
        CHECK(globals == 2 && j == 6);
        // the forward's plan of the same counts is what it was
        const ValPlan fw = plan_values(d);
        int dots = 0;
        for (int i = 0; i < fw.n; ++i) dots += fw.launch[i].kernel == VK_DOT;
        CHECK(fw.n == 7 && dots == 1);
    }

    if (failures) return 1;
    std::printf("gradplan ok\n");
    return 0;
}
