// valplan_smooth_check.cpp -- the launch plans of a smoothed values plan (csrc/mhs_valplan.hpp, csrc/mhs_smooth.hpp) on
// the host.  Such a plan holds two planes per C entry and classifies at sb = 2 x vb at width 1: its classes, needs and
// both launch plans are the width-2 plus-times plan's of the same type (the tables of tests/valplan_batched_check.cpp at
// sb 16, the FP64 width-1 table at sb 8), and every launch's dynamic bytes plus its kernel's static LDS -- asked at
// (vb, width 1): the smoothed kernels stage A values as the width-1 kernels do -- fits one workgroup's 160 KiB.
// Built by tests/test_smooth_host.py with -fsanitize=address,undefined; prints "valplan smooth ok".
#include "../mh-spgemm_amd/csrc/mhs_smooth.hpp"
#include "../mh-spgemm_amd/csrc/mhs_valplan.hpp"

#include <cstdio>
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

static bool same_launch(const ValLaunch& a, const ValLaunch& b) {
    return a.kernel == b.kernel && a.cls == b.cls && a.grid == b.grid && a.block == b.block && a.lds == b.lds &&
           a.region == b.region && a.count == b.count;
}

int main() {
    const int LDS_MAX = 163840;
    const long long WIDE = 1000000;
    for (int vb : {VAL_VB_F64, VAL_VB_F32}) {
        const int sb = val_sum_bytes(vb, 1 * val_smooth_planes(SMOOTH_LSE), VAL_ACC_NATIVE);
        CHECK(sb == 2 * vb && val_sb_ok(sb) && sb == val_sum_bytes(vb, 2, VAL_ACC_NATIVE));
        CHECK(val_sum_bytes(vb, 1 * val_smooth_planes(SMOOTH_NONE), VAL_ACC_NATIVE) == vb);
        // ---- every launch, every need: the width-2 plan's launches; dynamic bytes + the width-1 stage fit a workgroup
        for (int need : {0, 16, 48, 512, 768, 800, 1200, 1280, 8192, 8196, 32768, 32772, 100000, 159744}) {
            ValCounts c{};
            for (int k = VC_TEAM; k < VAL_NCLASS; ++k) {
                c.rows[k] = 10 * (k + 1);
                c.need[k] = need < val_class_cap(k, sb) ? need : val_class_cap(k, sb);
            }
            const ValPlan p = plan_values(c, sb), g = plan_grad(c, sb);
            const ValPlan w2 = plan_values(c, 2 * vb), gw2 = plan_grad(c, 2 * vb);
            CHECK(p.n == 7 && g.n == 7 && w2.n == 7 && gw2.n == 7);
            for (int i = 0; i < p.n; ++i) {
                const ValLaunch& l = p.launch[i];
                CHECK(same_launch(l, w2.launch[i]) && same_launch(g.launch[i], gw2.launch[i]));
                CHECK(l.lds >= 0 && l.lds + val_static_lds(l.kernel, vb, 1) <= LDS_MAX);
                CHECK(g.launch[i].lds + val_static_lds(g.launch[i].kernel, vb, 1) <= LDS_MAX);
                CHECK(l.region >= c.need[l.cls] && l.region <= val_class_cap(l.cls, sb));
                ValLaunch want = l;
                if (l.kernel == VK_DOT) want.kernel = VK_GLOBAL;
                CHECK(same_launch(g.launch[i], want));
            }
        }
        // at the caps: the block launch takes all that the width-1 stage leaves
        CHECK(val_static_lds(VK_BLOCK_DIRECT, vb, 1) == VAL_STAGE * (8 + vb) && VAL_BLOCK_BYTES + val_static_lds(VK_BLOCK_DIRECT, vb, 1) <= LDS_MAX);
        CHECK(WPB * VAL_WAVE_BYTES + val_static_lds(VK_WAVE_SEARCH, vb, 1) <= LDS_MAX);
        CHECK(val_static_lds(VK_DOT, vb, 1) == WPB * 64 * (4 + vb));
        CHECK(!val_team_registers(sb) && val_team_launch_cap(sb) + val_static_lds(VK_TEAM, vb, 1) <= VAL_LDS_PLAIN);
        // ---- two planes of vb and the one column array stay inside a slice the guards at sb accept
        for (int region = 0; region <= VAL_BLOCK_BYTES; region += (region < 16384 ? 1 : 61)) {
            const long long ne = val_slice_entries(region, sb);
            CHECK(2 * ne * vb + ne * 4 <= region);
            const long long top = region / sb;
            for (long long span : {1LL, top - 1, top, top + 1})
                if (val_slice_fits(span, region, sb)) CHECK(2 * span * vb <= region);
        }
    }
    // ---- the class edges: FP64 smoothed = the sb 16 table, FP32 smoothed = the FP64 width-1 table
    CHECK(val_wave_direct_span(16) == 512 && val_wave_search_n(16) == 408 && val_block_direct_span(16) == 9984 &&
          val_block_search_n(16) == 7986);
    CHECK(val_wave_direct_span(8) == 1024 && val_wave_search_n(8) == 682 && val_block_direct_span(8) == 19968 &&
          val_block_search_n(8) == 13312);
    CHECK(val_class(200, 512, 1000, 16) == VC_WAVE_DIRECT && val_class(200, 513, 1000, 16) == VC_BLOCK_DIRECT);
    CHECK(val_class(408, WIDE, 2000, 16) == VC_WAVE_SEARCH && val_class(409, WIDE, 2000, 16) == VC_BLOCK_SEARCH);
    CHECK(val_class(3000, 9984, 4000, 16) == VC_BLOCK_DIRECT && val_class(3000, 9985, 4000, 16) == VC_BLOCK_SEARCH);
    CHECK(val_class(7986, WIDE, 8000, 16) == VC_BLOCK_SEARCH && val_class(7987, WIDE, 8000, 16) == VC_GLOBAL);
    CHECK(val_class(200, 1024, 1000, 8) == VC_WAVE_DIRECT && val_class(200, 1025, 1000, 8) == VC_BLOCK_DIRECT);
    CHECK(val_class(682, WIDE, 2000, 8) == VC_WAVE_SEARCH && val_class(683, WIDE, 2000, 8) == VC_BLOCK_SEARCH);
    CHECK(val_class(13312, WIDE, 20000, 8) == VC_BLOCK_SEARCH && val_class(13313, WIDE, 20000, 8) == VC_GLOBAL);
    // every row of an LDS class at sb passes the two-plane guards on a slice of exactly its need
    for (int sb : {16, 8})
        for (int n = 1; n <= 14000; n += 7)
            for (long long span : {(long long)n, 2LL * n, 17LL * n, 512LL, 513LL, 1024LL, 1025LL, 9984LL, 19968LL, WIDE})
                for (long long prod : {1LL, 512LL, 513LL, 2048LL, 2049LL}) {
                    if (span < n) continue;
                    const int cls = val_class(n, span, prod, sb);
                    const int need = val_row_need(cls, n, span, sb);
                    CHECK(need <= val_class_cap(cls, sb));
                    if (cls == VC_WAVE_DIRECT || cls == VC_BLOCK_DIRECT) CHECK(val_slice_fits(span, need, sb));
                    else if (cls != VC_GLOBAL) CHECK(n <= val_slice_entries(need, sb));
                }
    if (failures) return 1;
    std::printf("valplan smooth ok\n");
    return 0;
}
