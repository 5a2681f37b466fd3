// valplan_mixed_check.cpp -- the launch plans of a mixed values plan (FP32 values, FP64 sums: csrc/mhs_valplan.hpp,
// ValAccum) on the host.  Such a plan of width W classifies and plans at sb = 8 W with a 4-byte value: for W = 1, 2
// and 4, every launch's dynamic bytes plus the kernel's static LDS at vb = 4 fits one workgroup; the float backward
// kernels' guards at W x 4 accept every row the forward's guards at sb accept, for regions up to the caps; and the
// team launch at W = 4 is the registered 73,728 B.
// Built by tests/test_values_mixed_host.py with -fsanitize=address,undefined; prints "valplan mixed ok".
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
    const int LDS_MAX = 163840, VB = VAL_VB_F32;
    // ---- the sum bytes: a mixed plan's are the FP64 plan's of its width, a native plan's its own
    CHECK(VAL_ACC_NATIVE == 0 && VAL_ACC_F64 == 1 && val_accum_ok(0) && val_accum_ok(1) && !val_accum_ok(-1) && !val_accum_ok(2));
    for (int W : {1, 2, 4}) {
        CHECK(val_sum_bytes(VAL_VB_F32, W, VAL_ACC_F64) == 8 * W && val_sum_bytes(VAL_VB_F64, W, VAL_ACC_F64) == 8 * W);
        CHECK(val_sum_bytes(VAL_VB_F32, W, VAL_ACC_NATIVE) == 4 * W && val_sum_bytes(VAL_VB_F64, W, VAL_ACC_NATIVE) == 8 * W);
        CHECK(val_sb_ok(val_sum_bytes(VAL_VB_F32, W, VAL_ACC_F64)));
    }

    for (int W : {1, 2, 4}) {
        const int sb = val_sum_bytes(VB, W, VAL_ACC_F64), fb = W * VB;  // the forward's guard bytes, the float backward's
        // ---- every launch, every need: dynamic bytes + the float stage fit one workgroup; the backward's list is the
        // forward's (dot rows on the global-form kernel), so the same sums hold for the float backward kernels
        for (int need : {0, 16, 48, 512, 768, 800, 1200, 1280, 2304, 8192, 8196, 32768, 32772, 100000, 159744}) {
            ValCounts c{};
            for (int k = VC_TEAM; k < VAL_NCLASS; ++k) {
                c.rows[k] = 10 * (k + 1);
                c.need[k] = need < val_class_cap(k, sb) ? need : val_class_cap(k, sb);
            }
            const ValPlan p = plan_values(c, sb), g = plan_grad(c, sb);
            CHECK(p.n == 7 && g.n == 7);
            for (int i = 0; i < p.n; ++i) {
                const ValLaunch& l = p.launch[i];
                CHECK(l.lds >= 0 && l.lds + val_static_lds(l.kernel, VB, W) <= LDS_MAX);
                CHECK(val_static_lds(l.kernel, VB, W) <= val_static_lds(l.kernel, VAL_VB_F64, W));  // (the stage holds floats)
                CHECK(l.region >= c.need[l.cls] && l.region <= val_class_cap(l.cls, sb));
                ValLaunch want = l;
                if (l.kernel == VK_DOT) want.kernel = VK_GLOBAL;
                CHECK(same_launch(g.launch[i], want));
                CHECK(g.launch[i].lds + val_static_lds(g.launch[i].kernel, VB, W) <= LDS_MAX);
                // the plan is the FP64 plan's of the same counts and width
                CHECK(same_launch(l, plan_values(c, W * VAL_VB_F64).launch[i]));
            }
        }
        // at the caps: the block launch takes all that the float stage leaves and more than it needs
        CHECK(VAL_BLOCK_BYTES + val_static_lds(VK_BLOCK_DIRECT, VB, W) <= LDS_MAX);
        CHECK(WPB * VAL_WAVE_BYTES + val_static_lds(VK_WAVE_SEARCH, VB, W) <= LDS_MAX);
        CHECK(val_team_launch_cap(sb) + val_static_lds(VK_TEAM, VB, W) <= LDS_MAX);
        CHECK(val_static_lds(VK_DOT, VB, W) == WPB * 64 * (4 + 4 * W));

        // ---- the float backward kernels' guards accept what the forward's accept, for every region up to the caps
        for (int region = 0; region <= VAL_BLOCK_BYTES; region += (region < 16384 ? 1 : 61)) {
            const int ne = val_slice_entries(region, sb);
            CHECK(val_slice_entries(region, fb) >= ne);
            // (the float layout of the entries the forward admits stays inside the region)
            CHECK((long long)ne * val_search_entry(fb) <= region);
            const long long top = region / sb;  // the widest span the forward admits
            for (long long span : {1LL, top - 1, top, top + 1, 2 * top, (long long)region / fb, (long long)region / fb + 1}) {
                if (val_slice_fits(span, region, sb)) CHECK(val_slice_fits(span, region, fb));
                if (val_slice_fits(span, region, fb)) CHECK(span * fb <= region);
            }
        }
        for (int region : {VAL_WAVE_BYTES, VAL_BLOCK_SMALL, VAL_BLOCK_BYTES, val_class_cap(VC_TEAM, sb)}) {
            CHECK(val_slice_entries(region, fb) >= val_slice_entries(region, sb));
            for (long long span = 1; span <= region / sb + 2; span += 1 + span / 97)
                CHECK(!val_slice_fits(span, region, sb) || val_slice_fits(span, region, fb));
        }
        // every row of an LDS class at sb passes the float guards on a slice of exactly its need
        for (int n = 1; n <= 14000; n += 5)
            for (long long span : {(long long)n, 2LL * n, 17LL * n, 256LL, 257LL, 1024LL, 1025LL, 4992LL, 19968LL, 1000000LL})
                for (long long prod : {1LL, 512LL, 513LL, 2048LL, 2049LL}) {
                    if (span < n) continue;
                    const int cls = val_class(n, span, prod, sb);
                    const int need = val_row_need(cls, n, span, sb);
                    if (cls == VC_WAVE_DIRECT || cls == VC_BLOCK_DIRECT) CHECK(val_slice_fits(span, need, fb));
                    else if (cls != VC_GLOBAL) CHECK(n <= val_slice_entries(need, fb));
                }
    }

    // ---- the team launch at W = 4: the registered 73,728 B, and no other width's is past the plain limit
    {
        const int sb = val_sum_bytes(VB, 4, VAL_ACC_F64);
        CHECK(sb == 32 && val_team_registers(sb) && val_team_launch_cap(sb) == 73728);
        ValCounts c{};
        c.rows[VC_TEAM] = 100;
        c.need[VC_TEAM] = (int)val_lds_search(VAL_TEAM_NMAX, sb);
        const ValPlan p = plan_values(c, sb), g = plan_grad(c, sb);
        CHECK(p.n == 1 && p.launch[0].kernel == VK_TEAM && p.launch[0].region == 2304 && p.launch[0].lds == 73728);
        CHECK(g.n == 1 && same_launch(g.launch[0], p.launch[0]));
        CHECK(p.launch[0].lds > VAL_LDS_PLAIN && p.launch[0].lds <= LDS_MAX);
        // (the float team kernels of width 4 alone would ask for 40,960 B: the backward registers the mixed launch too)
        CHECK(val_team_launch_cap(4 * VB) == 40960 && !val_team_registers(4 * VB));
        CHECK(!val_team_registers(val_sum_bytes(VB, 1, VAL_ACC_F64)) && !val_team_registers(val_sum_bytes(VB, 2, VAL_ACC_F64)));
    }

    if (failures) return 1;
    std::printf("valplan mixed ok\n");
    return 0;
}
