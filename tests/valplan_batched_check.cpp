// valplan_batched_check.cpp -- the values row classes and launch plans (csrc/mhs_valplan.hpp) as a function of the
// sum bytes sb = width x value size, on the host, for the widths of the batched plans: the four caps at sb 16 and
// 32 against the literals of the width table, rows one below, at and one above each cap through val_class,
// val_row_need and the slice guards at the exact byte, plan_values per class against hand-computed literals,
// static + dynamic LDS of every launch of every class, type and width within a workgroup's 163,840 B, the team
// launch at sb = 32 against what its kernel is registered for, and sb 4 and 8 against the existing signatures.
// Built by tests/test_values_batched_host.py with -fsanitize=address,undefined; prints "valplan batched ok".
#include "../mh-spgemm_amd/csrc/mhs_valplan.hpp"

#include <cstdio>
#include <cstdlib>
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

static bool same_launch(const ValLaunch& a, const ValLaunch& b) {
    return a.kernel == b.kernel && a.cls == b.cls && a.grid == b.grid && a.block == b.block && a.lds == b.lds &&
           a.region == b.region && a.count == b.count;
}

// The caps of one sb: wave-direct span, wave-search n, block-direct span, block-search n
struct Caps {
    int sb, wd, ws, bd, bs;
};

int main() {
    const long long WIDE = 1000000;  // a span no direct class holds
    CHECK(VAL_WIDTH_MAX == 4 && val_width_ok(1) && val_width_ok(2) && val_width_ok(4) && !val_width_ok(0) && !val_width_ok(3) &&
          !val_width_ok(8) && !val_width_ok(-1));
    CHECK(val_sb_ok(4) && val_sb_ok(8) && val_sb_ok(16) && val_sb_ok(32) && !val_sb_ok(0) && !val_sb_ok(12) && !val_sb_ok(64));
    CHECK(val_vb_ok(4) && val_vb_ok(8) && !val_vb_ok(16) && !val_vb_ok(32));  // (a value is still 4 or 8 bytes)
    CHECK(val_search_entry(16) == 20 && val_search_entry(32) == 36);           // W sums and the one shared column

    // ---- the width table
    const Caps table[] = {{4, 2048, 1024, 39936, 19968}, {8, 1024, 682, 19968, 13312}, {16, 512, 408, 9984, 7986},
                          {32, 256, 226, 4992, 4436}};
    for (const Caps& t : table) {
        CHECK(val_wave_direct_span(t.sb) == t.wd && val_wave_search_n(t.sb) == t.ws);
        CHECK(val_block_direct_span(t.sb) == t.bd && val_block_search_n(t.sb) == t.bs);
        // each cap is the last that fits its slice
        CHECK(val_lds_direct(t.wd, t.sb) <= VAL_WAVE_BYTES && val_lds_direct(t.wd + 1, t.sb) > VAL_WAVE_BYTES);
        CHECK(val_lds_search(t.ws, t.sb) <= VAL_WAVE_BYTES && val_lds_search(t.ws + 1, t.sb) > VAL_WAVE_BYTES);
        CHECK(val_lds_direct(t.bd, t.sb) <= VAL_BLOCK_BYTES && val_lds_direct(t.bd + 1, t.sb) > VAL_BLOCK_BYTES);
        CHECK(val_lds_search(t.bs, t.sb) <= VAL_BLOCK_BYTES && val_lds_search(t.bs + 1, t.sb) > VAL_BLOCK_BYTES);
    }

    // ---- rows one below, at and one above each cap (the rows of tests/test_gpu_values_batched.py's edges)
    // sb = 16
    CHECK(val_class(200, 511, 1000, 16) == VC_WAVE_DIRECT && val_class(200, 512, 1000, 16) == VC_WAVE_DIRECT);
    CHECK(val_class(200, 513, 1000, 16) == VC_BLOCK_DIRECT);
    CHECK(val_class(407, WIDE, 2000, 16) == VC_WAVE_SEARCH && val_class(408, WIDE, 2000, 16) == VC_WAVE_SEARCH);
    CHECK(val_class(409, WIDE, 2000, 16) == VC_BLOCK_SEARCH);
    CHECK(val_class(3000, 9983, 4000, 16) == VC_BLOCK_DIRECT && val_class(3000, 9984, 4000, 16) == VC_BLOCK_DIRECT);
    CHECK(val_class(3000, 9985, 4000, 16) == VC_BLOCK_SEARCH);
    CHECK(val_class(7985, WIDE, 8000, 16) == VC_BLOCK_SEARCH && val_class(7986, WIDE, 8000, 16) == VC_BLOCK_SEARCH);
    CHECK(val_class(7987, WIDE, 8000, 16) == VC_GLOBAL);
    // sb = 32
    CHECK(val_class(200, 255, 1000, 32) == VC_WAVE_DIRECT && val_class(200, 256, 1000, 32) == VC_WAVE_DIRECT);
    CHECK(val_class(200, 257, 1000, 32) == VC_BLOCK_DIRECT);
    CHECK(val_class(225, WIDE, 2000, 32) == VC_WAVE_SEARCH && val_class(226, WIDE, 2000, 32) == VC_WAVE_SEARCH);
    CHECK(val_class(227, WIDE, 2000, 32) == VC_BLOCK_SEARCH);
    CHECK(val_class(3000, 4991, 4000, 32) == VC_BLOCK_DIRECT && val_class(3000, 4992, 4000, 32) == VC_BLOCK_DIRECT);
    CHECK(val_class(3000, 4993, 4000, 32) == VC_BLOCK_SEARCH);
    CHECK(val_class(4435, WIDE, 4500, 32) == VC_BLOCK_SEARCH && val_class(4436, WIDE, 4500, 32) == VC_BLOCK_SEARCH);
    CHECK(val_class(4437, WIDE, 4500, 32) == VC_GLOBAL);
    // their needs and the slice guards at the exact byte
    for (const Caps& t : table) {
        const int sb = t.sb;
        CHECK(val_row_need(VC_WAVE_DIRECT, 200, t.wd, sb) == VAL_WAVE_BYTES);
        CHECK(val_row_need(VC_BLOCK_DIRECT, 3000, t.wd + 1, sb) == VAL_WAVE_BYTES + sb);
        CHECK(val_row_need(VC_BLOCK_DIRECT, 3000, t.bd, sb) == VAL_BLOCK_BYTES);
        CHECK(val_row_need(VC_WAVE_SEARCH, t.ws, WIDE, sb) == (sb + 4) * t.ws && (sb + 4) * t.ws <= VAL_WAVE_BYTES);
        CHECK(val_row_need(VC_BLOCK_SEARCH, t.ws + 1, WIDE, sb) == (sb + 4) * (t.ws + 2));  // (n rounded to even)
        CHECK(val_row_need(VC_BLOCK_SEARCH, t.bs, WIDE, sb) == (sb + 4) * t.bs && (sb + 4) * t.bs <= VAL_BLOCK_BYTES);
        CHECK(val_row_need(VC_TEAM, 64, 100, sb) == (sb + 4) * 64 && val_row_need(VC_TEAM, 5, 100, sb) == (sb + 4) * 6);
        CHECK(val_row_need(VC_GLOBAL, 9000, WIDE, sb) == 0 && val_row_need(VC_DOT, 5, 5, sb) == 0);
        CHECK(val_slice_fits(t.wd, VAL_WAVE_BYTES, sb) && !val_slice_fits(t.wd + 1, VAL_WAVE_BYTES, sb) &&
              !val_slice_fits(t.wd, VAL_WAVE_BYTES - 1, sb));
        CHECK(val_slice_fits(t.bd, VAL_BLOCK_BYTES, sb) && !val_slice_fits(t.bd + 1, VAL_BLOCK_BYTES, sb) &&
              !val_slice_fits(t.bd, VAL_BLOCK_BYTES - 1, sb));
        CHECK(val_slice_entries(VAL_WAVE_BYTES, sb) >= t.ws && val_slice_entries(VAL_WAVE_BYTES, sb) <= t.ws + 1);
        CHECK(val_slice_entries(VAL_BLOCK_BYTES, sb) >= t.bs && val_slice_entries(VAL_BLOCK_BYTES, sb) <= t.bs + 1);
        CHECK(val_slice_entries((sb + 4) * 64, sb) == 64 && val_slice_entries((sb + 4) * 64 - 1, sb) == 63);
        CHECK(val_slice_entries(0, sb) == 0 && val_slice_entries(sb + 3, sb) == 0 && val_slice_entries(sb + 4, sb) == 1);
        CHECK(val_slice_fits(1, sb, sb) && !val_slice_fits(1, sb - 1, sb) && !val_slice_fits(0, 8192, sb) &&
              !val_slice_fits(0x7fffffffffffLL, 8192, sb));
        // W sum planes of `pitch` entries and the one column array behind them stay inside the region
        for (int region : {sb + 4, 2 * (sb + 4), 1280, 2304, 8192, 32768, 159744}) {
            const long long ne = val_slice_entries(region, sb);
            CHECK(ne * sb + ne * 4 <= region);
        }
    }
    CHECK(val_slice_entries(8192, 16) == 409 && val_slice_entries(8192, 32) == 227);
    CHECK(val_slice_entries(159744, 16) == 7987 && val_slice_entries(159744, 32) == 4437);
    // a guard of the wrong width on a launch would overrun or skip: the widths differ at one region
    CHECK(val_slice_fits(512, 8192, 16) && !val_slice_fits(512, 8192, 32) && val_slice_entries(8192, 16) != val_slice_entries(8192, 8));
    // every row fits what its class may declare, and passes the guard of a slice of exactly its need
    for (int sb : {16, 32})
        for (int n = 1; n <= 9000; n += 7)
            for (long long span : {(long long)n, 2LL * n, 17LL * n, 256LL, 257LL, 512LL, 513LL, 4992LL, 4993LL, 9984LL, 9985LL, WIDE})
                for (long long prod : {0LL, 1LL, 512LL, 513LL, 2048LL, 2049LL}) {
                    if (span < n) continue;
                    const int cls = val_class(n, span, prod, sb);
                    CHECK(cls > VC_NONE && cls < VC_COUNT);
                    const int need = val_row_need(cls, n, span, sb);
                    CHECK(need <= val_class_cap(cls, sb));
                    if (cls == VC_WAVE_DIRECT || cls == VC_BLOCK_DIRECT) {
                        CHECK(val_slice_fits(span, need, sb) && !val_slice_fits(span, need - 1, sb));
                    } else if (cls != VC_GLOBAL) {
                        CHECK(n <= val_slice_entries(need, sb));
                    }
                }
    // ---- counts do not move with the width: the team edges, the wave product cap, the dense ratio
    for (int sb : {4, 8, 16, 32}) {
        CHECK(val_class(0, 0, 100, sb) == VC_NONE);
        CHECK(val_class(64, 100, 200, sb) == VC_TEAM && val_class(65, 100, 200, sb) == VC_WAVE_DIRECT);
        CHECK(val_class(10, 50, 512, sb) == VC_TEAM && val_class(10, 50, 513, sb) == VC_WAVE_DIRECT);
        CHECK(val_class(64, 100, 0, sb) == VC_TEAM && val_class(65, 100, 0, sb) == VC_GLOBAL);
        CHECK(val_class(100, 200, 2048, sb) == VC_WAVE_DIRECT && val_class(100, 200, 2049, sb) == VC_BLOCK_DIRECT);
        CHECK(val_class(100, WIDE, 2048, sb) == VC_WAVE_SEARCH && val_class(100, WIDE, 2049, sb) == VC_BLOCK_SEARCH);
        // the dot class is chosen by counts: the same rows take it at every width
        for (int form : {VM_AUTO, VM_PRODUCT, VM_DOT})
            for (long long cost : {0LL, 10LL, 100000LL})
                for (long long prod : {0LL, 100LL, 100000LL}) {
                    const int m = val_class_masked(300, WIDE, prod, 3, cost, form, VAL_DOT_RATIO, sb);
                    CHECK((m == VC_DOT) == (val_class_masked(300, WIDE, prod, 3, cost, form) == VC_DOT));
                    if (m != VC_DOT) CHECK(m == val_class(300, WIDE, prod, sb));
                }
    }

    // ---- sb 4 and 8 are the existing signatures
    for (int n : {0, 1, 63, 64, 65, 100, 681, 682, 683, 1024, 1025, 3000, 13312, 13313, 19968, 19969, 30000})
        for (long long span : {1LL, 100LL, 1023LL, 1024LL, 1025LL, 2048LL, 2049LL, 19968LL, 19969LL, 39936LL, 39937LL, WIDE})
            for (long long prod : {0LL, 1LL, 512LL, 513LL, 2048LL, 2049LL, 100000LL}) {
                const int cls = val_class(n, span, prod);
                CHECK(val_class(n, span, prod, 8) == cls && val_class(n, span, prod, VAL_VB_F64) == cls);
                CHECK(val_row_need(cls, n, span, 8) == val_row_need(cls, n, span));
                CHECK(val_class(n, span, prod, 4) == val_class(n, span, prod, VAL_VB_F32));
            }
    for (int c = 0; c < VAL_NCLASS; ++c) CHECK(val_class_cap(c, 8) == val_class_cap(c));
    CHECK(VAL_WAVE_DIRECT_SPAN == 1024 && VAL_WAVE_SEARCH_N == 682 && VAL_BLOCK_DIRECT_SPAN == 19968 && VAL_BLOCK_SEARCH_N == 13312);
    CHECK(val_caps_fit(4) && val_caps_fit(8));
    {
        ValCounts c{};
        for (int k = VC_TEAM; k < VAL_NCLASS; ++k) {
            c.rows[k] = 7 * k;
            c.need[k] = val_class_cap(k) / 2;
        }
        const ValPlan a = plan_values(c), b = plan_values(c, 8);
        CHECK(a.n == b.n);
        for (int i = 0; i < a.n; ++i) CHECK(same_launch(a.launch[i], b.launch[i]));
    }

    // ---- the team launch: past 64 KiB at sb = 32 only, and then what its kernel is registered for
    CHECK(VAL_LDS_PLAIN == 65536);
    CHECK(val_team_launch_cap(4) == 16384 && val_team_launch_cap(8) == 24576 && val_team_launch_cap(16) == 40960 &&
          val_team_launch_cap(32) == 73728);
    CHECK(!val_team_registers(4) && !val_team_registers(8) && !val_team_registers(16) && val_team_registers(32));
    CHECK(val_class_cap(VC_TEAM, 16) == 1280 && val_class_cap(VC_TEAM, 32) == 2304);
    for (int sb : {4, 8, 16, 32})
        for (int need : {0, sb + 4, 6 * (sb + 4), 63 * (sb + 4), 64 * (sb + 4)}) {
            const ValPlan p = plan_values(one(VC_TEAM, 100, need), sb);
            CHECK(p.n == 1 && p.launch[0].lds == VAL_TEAM_ROWS * p.launch[0].region);
            CHECK(p.launch[0].lds <= val_team_launch_cap(sb));                           // never past the registration
            CHECK(val_team_registers(sb) || p.launch[0].lds <= VAL_LDS_PLAIN);           // unregistered: a plain launch
            CHECK(p.launch[0].region % (2 * (sb + 4)) == 0 && p.launch[0].region >= need);
            CHECK(val_slice_entries(p.launch[0].region, sb) >= need / (sb + 4));
        }

    // ---- plan_values per class at sb 16 and 32 against literals
    {
        const ValPlan p = plan_values(one(VC_TEAM, 1, 2304), 32);
        CHECK(p.n == 1 && p.launch[0].kernel == VK_TEAM && p.launch[0].cls == VC_TEAM && p.launch[0].grid == 1 &&
              p.launch[0].block == 256 && p.launch[0].region == 2304 && p.launch[0].lds == 73728 && p.launch[0].count == 1);
        const ValPlan q = plan_values(one(VC_TEAM, 33, 216), 32);  // n 5 or 6: 36 B x 6
        CHECK(q.launch[0].grid == 2 && q.launch[0].region == 216 && q.launch[0].lds == 6912);
        const ValPlan r = plan_values(one(VC_TEAM, 33, 1280), 16);  // n 64: 20 B x 64
        CHECK(r.launch[0].region == 1280 && r.launch[0].lds == 40960);
        const ValPlan z = plan_values(one(VC_TEAM, 33, 0), 16);  // no need counted: the cap
        CHECK(z.launch[0].region == 1280);
    }
    for (int sb : {16, 32}) {
        const ValPlan p = plan_values(one(VC_WAVE_DIRECT, 5, 200 * sb), sb);  // span 200
        CHECK(p.n == 1 && p.launch[0].kernel == VK_WAVE_DIRECT && p.launch[0].grid == 2 && p.launch[0].block == 256 &&
              p.launch[0].region == (sb == 16 ? 3328 : 6400) && p.launch[0].lds == 4 * p.launch[0].region);
        const ValPlan q = plan_values(one(VC_WAVE_DIRECT, 1, 8192), sb);  // the cap
        CHECK(q.launch[0].grid == 1 && q.launch[0].region == 8192 && q.launch[0].lds == 32768);
        const ValPlan s = plan_values(one(VC_WAVE_SEARCH, 9, (sb + 4) * 100), sb);  // n 100
        CHECK(s.n == 1 && s.launch[0].kernel == VK_WAVE_SEARCH && s.launch[0].grid == 3 && s.launch[0].block == 256 &&
              s.launch[0].region == (sb == 16 ? 2048 : 3840) && s.launch[0].lds == 4 * s.launch[0].region);
        const ValPlan bd = plan_values(one(VC_BLOCK_DIRECT, 3, (VAL_WAVE_BYTES / sb + 1) * sb), sb);  // one column past a wave
        CHECK(bd.n == 1 && bd.launch[0].kernel == VK_BLOCK_DIRECT && bd.launch[0].grid == 3 && bd.launch[0].block == 256 &&
              bd.launch[0].lds == 10240 && bd.launch[0].region == 10240);
        const ValPlan bb = plan_values(one(VC_BLOCK_DIRECT, 1, VAL_BLOCK_BYTES), sb);  // the cap
        CHECK(bb.launch[0].block == 1024 && bb.launch[0].lds == 159744 && bb.launch[0].region == 159744);
        CHECK(plan_values(one(VC_BLOCK_DIRECT, 1, 32768), sb).launch[0].block == 256);
        CHECK(plan_values(one(VC_BLOCK_DIRECT, 1, 32768 + sb), sb).launch[0].block == 1024);
        const ValPlan bs = plan_values(one(VC_BLOCK_SEARCH, 2, (sb + 4) * val_block_search_n(sb)), sb);  // the cap
        CHECK(bs.n == 1 && bs.launch[0].kernel == VK_BLOCK_SEARCH && bs.launch[0].grid == 2 && bs.launch[0].block == 1024 &&
              bs.launch[0].lds == 159744 && bs.launch[0].region == 159744);
        const ValPlan g = plan_values(one(VC_GLOBAL, 1, 0), sb);
        CHECK(g.n == 1 && g.launch[0].kernel == VK_GLOBAL && g.launch[0].grid == 1 && g.launch[0].block == 1024 &&
              g.launch[0].lds == 0);
        const ValPlan d = plan_values(one(VC_DOT, 9, 0), sb);
        CHECK(d.n == 1 && d.launch[0].kernel == VK_DOT && d.launch[0].cls == VC_DOT && d.launch[0].grid == 3 &&
              d.launch[0].block == 256 && d.launch[0].lds == 0);
    }

    // ---- every class at once, every need, every type and width: static + dynamic LDS within one workgroup
    CHECK(LDS_MAX_C == 163840);
    for (int vb : {4, 8})
        for (int width : {1, 2, 4}) {
            const int sb = width * vb;
            CHECK(val_sb_ok(sb));
            // the static part: the stage of A entries (1 KiB a wave, VAL_STAGE_BYTES a block), the dot stage
            CHECK(val_static_lds(VK_TEAM, vb, width) == 0 && val_static_lds(VK_GLOBAL, vb, width) == 0);
            CHECK(val_static_lds(VK_WAVE_DIRECT, vb, width) == val_static_lds(VK_WAVE_SEARCH, vb, width) &&
                  val_static_lds(VK_WAVE_DIRECT, vb, width) <= WPB * 1024);
            CHECK(val_static_lds(VK_BLOCK_DIRECT, vb, width) == val_static_lds(VK_BLOCK_SEARCH, vb, width) &&
                  val_static_lds(VK_BLOCK_DIRECT, vb, width) <= VAL_STAGE_BYTES);
            CHECK(val_static_lds(VK_DOT, vb, width) == 256 * (4 + sb));
            if (width > 1) CHECK(val_static_lds(VK_WAVE_DIRECT, vb, width) == 2048 && val_static_lds(VK_BLOCK_DIRECT, vb, width) == 2048);
            for (int need : {0, 16, 48, 216, 512, 800, 1200, 2304, 8192, 8196, 32768, 32772, 100000, 159744}) {
                ValCounts c{};
                for (int k = VC_TEAM; k < VAL_NCLASS; ++k) {
                    c.rows[k] = 10 * (k + 1);
                    c.need[k] = need < val_class_cap(k, sb) ? need : val_class_cap(k, sb);
                }
                const ValPlan p = plan_values(c, sb);
                CHECK(p.n == 7);
                const int order[7] = {VC_DOT, VC_GLOBAL, VC_BLOCK_SEARCH, VC_BLOCK_DIRECT, VC_WAVE_SEARCH, VC_WAVE_DIRECT, VC_TEAM};
                for (int i = 0; i < 7 && i < p.n; ++i) {
                    const ValLaunch& l = p.launch[i];
                    CHECK(l.cls == order[i] && l.count == c.rows[order[i]]);
                    CHECK(l.lds >= 0 && l.lds + val_static_lds(l.kernel, vb, width) <= 163840);
                    CHECK(l.region >= c.need[l.cls] && l.region <= val_class_cap(l.cls, sb));
                    if (l.cls == VC_BLOCK_DIRECT || l.cls == VC_BLOCK_SEARCH) {
                        CHECK(l.lds == l.region && (l.block == 256) == (l.lds <= 32768) && l.lds <= VAL_BLOCK_BYTES);
                    } else if (l.cls == VC_WAVE_DIRECT || l.cls == VC_WAVE_SEARCH) {
                        CHECK(l.block == 256 && l.lds == 4 * l.region && l.lds <= 32768);
                    } else if (l.cls == VC_TEAM) {
                        CHECK(l.block == 256 && l.lds == 32 * l.region && l.lds <= val_team_launch_cap(sb));
                    } else {
                        CHECK(l.lds == 0);
                    }
                }
            }
        }

    if (failures) return 1;
    std::printf("valplan batched ok\n");
    return 0;
}
