// gradplan_batched_check.cpp -- the launch plan of the batched values backward (plan_grad(counts, sb),
// csrc/mhs_valplan.hpp) on the host, as a function of the sum bytes sb = width x value size: per class at sb 16 and
// 32 against hand-computed literals, the dot rows routed to the global-form kernel with the rest of the list
// unchanged, static + dynamic LDS of every launch of every class, type and width within a workgroup's 163,840 B,
// the team launch at sb = 32 against what k_grad_team<double, 4> is registered for, and sb 4 and 8 against what
// tests/gradplan_check.cpp holds.  Built by tests/test_values_grad_batched_host.py with
// -fsanitize=address,undefined; prints "gradplan batched ok".
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

static bool is(const ValLaunch& l, int kernel, int cls, int grid, int block, int lds, int region, int count) {
    return l.kernel == kernel && l.cls == cls && l.grid == grid && l.block == block && l.lds == lds && l.region == region &&
           l.count == count;
}

int main() {
    // ---- no rows: no launch, at any sb
    for (int sb : {4, 8, 16, 32}) CHECK(plan_grad(ValCounts{}, sb).n == 0);

    // ---- per class at sb 16 and 32 against literals
    {
        const ValPlan p = plan_grad(one(VC_TEAM, 1, 2304), 32);  // n 64: 36 B x 64 a row, 32 rows a block
        CHECK(p.n == 1 && is(p.launch[0], VK_TEAM, VC_TEAM, 1, 256, 73728, 2304, 1));
        const ValPlan q = plan_grad(one(VC_TEAM, 33, 216), 32);  // n 5 or 6: 36 B x 6
        CHECK(q.n == 1 && is(q.launch[0], VK_TEAM, VC_TEAM, 2, 256, 6912, 216, 33));
        const ValPlan r = plan_grad(one(VC_TEAM, 33, 1280), 16);  // n 64: 20 B x 64
        CHECK(r.n == 1 && is(r.launch[0], VK_TEAM, VC_TEAM, 2, 256, 40960, 1280, 33));
        const ValPlan z = plan_grad(one(VC_TEAM, 33, 0), 16);  // no need counted: the cap
        CHECK(z.n == 1 && z.launch[0].region == 1280 && z.launch[0].lds == 40960);
    }
    {
        // span 200 in a wave: 3200 B at sb 16 -> 3328 (256 B steps), 6400 B at sb 32
        CHECK(is(plan_grad(one(VC_WAVE_DIRECT, 5, 3200), 16).launch[0], VK_WAVE_DIRECT, VC_WAVE_DIRECT, 2, 256, 13312, 3328, 5));
        CHECK(is(plan_grad(one(VC_WAVE_DIRECT, 5, 6400), 32).launch[0], VK_WAVE_DIRECT, VC_WAVE_DIRECT, 2, 256, 25600, 6400, 5));
        // n 100 searched: 2000 B at sb 16 -> 2048, 3600 B at sb 32 -> 3840
        CHECK(is(plan_grad(one(VC_WAVE_SEARCH, 9, 2000), 16).launch[0], VK_WAVE_SEARCH, VC_WAVE_SEARCH, 3, 256, 8192, 2048, 9));
        CHECK(is(plan_grad(one(VC_WAVE_SEARCH, 9, 3600), 32).launch[0], VK_WAVE_SEARCH, VC_WAVE_SEARCH, 3, 256, 15360, 3840, 9));
        // one column past a wave's span: 8208 B at sb 16, 8224 B at sb 32 -> 10240 (2 KiB steps), 256 threads
        CHECK(is(plan_grad(one(VC_BLOCK_DIRECT, 3, 8208), 16).launch[0], VK_BLOCK_DIRECT, VC_BLOCK_DIRECT, 3, 256, 10240, 10240, 3));
        CHECK(is(plan_grad(one(VC_BLOCK_DIRECT, 3, 8224), 32).launch[0], VK_BLOCK_DIRECT, VC_BLOCK_DIRECT, 3, 256, 10240, 10240, 3));
        for (int sb : {16, 32}) {
            CHECK(is(plan_grad(one(VC_WAVE_DIRECT, 1, 8192), sb).launch[0], VK_WAVE_DIRECT, VC_WAVE_DIRECT, 1, 256, 32768, 8192, 1));
            CHECK(is(plan_grad(one(VC_BLOCK_DIRECT, 1, 159744), sb).launch[0], VK_BLOCK_DIRECT, VC_BLOCK_DIRECT, 1, 1024, 159744,
                     159744, 1));
            CHECK(plan_grad(one(VC_BLOCK_DIRECT, 1, 32768), sb).launch[0].block == 256);
            CHECK(plan_grad(one(VC_BLOCK_DIRECT, 1, 32768 + sb), sb).launch[0].block == 1024);
            CHECK(is(plan_grad(one(VC_BLOCK_SEARCH, 2, (sb + 4) * val_block_search_n(sb)), sb).launch[0], VK_BLOCK_SEARCH,
                     VC_BLOCK_SEARCH, 2, 1024, 159744, 159744, 2));
            CHECK(is(plan_grad(one(VC_GLOBAL, 1, 0), sb).launch[0], VK_GLOBAL, VC_GLOBAL, 1, 1024, 0, 0, 1));
            // the dot rows: the global-form kernel on the dot list, a wave per row; never VK_DOT
            CHECK(is(plan_grad(one(VC_DOT, 9, 0), sb).launch[0], VK_GLOBAL, VC_DOT, 3, 256, 0, 0, 9));
        }
    }

    // ---- every class at once, every need, every type and width
    CHECK(LDS_MAX_C == 163840);
    for (int vb : {4, 8})
        for (int width : {1, 2, 4}) {
            const int sb = width * vb;
            for (int need : {0, 16, 48, 216, 512, 800, 1200, 2304, 8192, 8196, 32768, 32772, 100000, 159744}) {
                ValCounts c{};
                for (int k = VC_TEAM; k < VAL_NCLASS; ++k) {
                    c.rows[k] = 10 * (k + 1);
                    c.need[k] = need < val_class_cap(k, sb) ? need : val_class_cap(k, sb);
                }
                const ValPlan p = plan_grad(c, sb), f = plan_values(c, sb);
                CHECK(p.n == 7 && f.n == 7);
                int globals = 0;
                for (int i = 0; i < 7 && i < p.n; ++i) {
                    const ValLaunch &l = p.launch[i], &m = f.launch[i];
                    // the forward's list, launch by launch; only the dot rows' kernel differs
                    CHECK(l.cls == m.cls && l.grid == m.grid && l.block == m.block && l.lds == m.lds && l.region == m.region &&
                          l.count == m.count);
                    CHECK(l.kernel != VK_DOT && (l.kernel == m.kernel) == (m.kernel != VK_DOT));
                    if (m.kernel == VK_DOT) CHECK(l.kernel == VK_GLOBAL && l.cls == VC_DOT && l.block == 256 && l.lds == 0);
                    globals += l.kernel == VK_GLOBAL;
                    // static + dynamic LDS within one workgroup (the backward's stages are the forward's: val_static_lds)
                    CHECK(l.lds >= 0 && l.lds + val_static_lds(l.kernel, vb, width) <= 163840);
                    CHECK(l.region >= c.need[l.cls] && l.region <= val_class_cap(l.cls, sb));
                    if (l.kernel == VK_TEAM) {
                        CHECK(l.lds == VAL_TEAM_ROWS * l.region && l.lds <= val_team_launch_cap(sb));
                        CHECK(val_team_registers(sb) || l.lds <= VAL_LDS_PLAIN);  // unregistered: a plain launch
                    }
                    if (l.cls == VC_BLOCK_DIRECT || l.cls == VC_BLOCK_SEARCH)
                        CHECK(l.lds == l.region && (l.block == 256) == (l.lds <= VAL_BLOCK_SMALL) && l.lds <= VAL_BLOCK_BYTES);
                    if (l.cls == VC_WAVE_DIRECT || l.cls == VC_WAVE_SEARCH) CHECK(l.lds == WPB * l.region && l.lds <= 32768);
                }
                CHECK(globals == 2);
            }
        }

    // ---- the sb = 32 team launch: 73,728 B, what the FP64 width-4 team kernel is registered for, and the only one
    CHECK(val_team_launch_cap(32) == 73728 && val_team_registers(32));
    CHECK(!val_team_registers(4) && !val_team_registers(8) && !val_team_registers(16));
    CHECK(plan_grad(one(VC_TEAM, 100, 64 * 36), 32).launch[0].lds == 73728);
    CHECK(plan_grad(one(VC_TEAM, 100, 64 * 20), 16).launch[0].lds == 40960);

    // ---- sb 4 and 8: what tests/gradplan_check.cpp holds (its literals again at sb = 8, by the default argument
    // and named; sb = 4 against the FP32 figures)
    {
        ValCounts c{};
        for (int k = 0; k < VC_COUNT; ++k) {
            c.rows[k] = 10 * (k + 1);
            c.need[k] = val_class_cap(k);
        }
        const ValPlan a = plan_grad(c), b = plan_grad(c, 8), d = plan_grad(c, VAL_VB_F64);
        const int order[6] = {VC_GLOBAL, VC_BLOCK_SEARCH, VC_BLOCK_DIRECT, VC_WAVE_SEARCH, VC_WAVE_DIRECT, VC_TEAM};
        const int grid[6] = {70, 60, 50, 10, 8, 1}, block[6] = {1024, 1024, 1024, 256, 256, 256};
        const int lds[6] = {0, 159744, 159744, 32768, 32768, 24576};
        const int region[6] = {0, 159744, 159744, 8192, 8192, 768};
        CHECK(a.n == 6 && b.n == 6 && d.n == 6);
        for (int i = 0; i < 6 && i < a.n; ++i) {
            CHECK(a.launch[i].cls == order[i] && a.launch[i].grid == grid[i] && a.launch[i].block == block[i] &&
                  a.launch[i].lds == lds[i] && a.launch[i].region == region[i]);
            CHECK(std::memcmp(&a.launch[i], &b.launch[i], sizeof(ValLaunch)) == 0);
            CHECK(std::memcmp(&a.launch[i], &d.launch[i], sizeof(ValLaunch)) == 0);
        }
        ValCounts s{};
        s.rows[VC_BLOCK_DIRECT] = 5000, s.need[VC_BLOCK_DIRECT] = 30000;
        s.rows[VC_WAVE_SEARCH] = 9, s.need[VC_WAVE_SEARCH] = 1000;
        s.rows[VC_TEAM] = 33, s.need[VC_TEAM] = 100;
        const ValPlan q = plan_grad(s, 8);
        CHECK(q.n == 3 && is(q.launch[0], VK_BLOCK_DIRECT, VC_BLOCK_DIRECT, 4096, 256, 30720, 30720, 5000));
        CHECK(is(q.launch[1], VK_WAVE_SEARCH, VC_WAVE_SEARCH, 3, 256, 4096, 1024, 9));
        CHECK(is(q.launch[2], VK_TEAM, VC_TEAM, 2, 256, 32 * 120, 120, 33));
        const ValPlan r = plan_grad(s, 4);  // FP32: a team row's slice in 16 B steps (2 entries of 8 B)
        CHECK(r.n == 3 && is(r.launch[0], VK_BLOCK_DIRECT, VC_BLOCK_DIRECT, 4096, 256, 30720, 30720, 5000));
        CHECK(is(r.launch[1], VK_WAVE_SEARCH, VC_WAVE_SEARCH, 3, 256, 4096, 1024, 9));
        CHECK(is(r.launch[2], VK_TEAM, VC_TEAM, 2, 256, 32 * 112, 112, 33));
    }

    if (failures) return 1;
    std::printf("gradplan batched ok\n");
    return 0;
}
