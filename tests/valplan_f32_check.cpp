// valplan_f32_check.cpp -- the values row classes and launch plans (csrc/mhs_valplan.hpp) as a function of the
// value size vb, on the host: the class of rows one below, at and one above every FP32 threshold, that vb = 8
// is what the signatures without vb return, each class's LDS need and cap, plan_values' and plan_grad's FP32
// launches against hand-computed literals, and the guards of a row's LDS slice at the exact byte.
// Built by tests/test_values_f32_host.py with -fsanitize=address,undefined; prints "valplan f32 ok".
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

int main() {
    const long long WIDE = 1000000;  // a span no direct class holds
    const int F32 = 4, F64 = 8;
    CHECK(VAL_VB_F32 == 4 && VAL_VB_F64 == 8 && val_vb_ok(4) && val_vb_ok(8) && !val_vb_ok(2) && !val_vb_ok(0));
    CHECK(val_search_entry(F32) == 8 && val_search_entry(F64) == 12);

    // ---- the FP32 caps follow from the LDS arithmetic
    CHECK(val_wave_direct_span(F32) == 2048 && val_wave_search_n(F32) == 1024);
    CHECK(val_block_direct_span(F32) == 39936 && val_block_search_n(F32) == 19968);
    CHECK(val_wave_direct_span(F64) == 1024 && val_wave_search_n(F64) == 682);
    CHECK(val_block_direct_span(F64) == 19968 && val_block_search_n(F64) == 13312);

    // ---- wave-direct: span <= 2048 (8 KiB of FP32 sums); past it 2049 <= 16 * 200: a block's direct table
    CHECK(val_class(200, 2047, 1000, F32) == VC_WAVE_DIRECT);
    CHECK(val_class(200, 2048, 1000, F32) == VC_WAVE_DIRECT);
    CHECK(val_class(200, 2049, 1000, F32) == VC_BLOCK_DIRECT);
    CHECK(val_class(200, 2048, 1000, F64) == VC_BLOCK_DIRECT);  // (FP64: a wave holds 1024)
    // ---- wave-search: n <= 1024 (8 B per entry in 8 KiB)
    CHECK(val_class(1023, WIDE, 2000, F32) == VC_WAVE_SEARCH);
    CHECK(val_class(1024, WIDE, 2000, F32) == VC_WAVE_SEARCH);
    CHECK(val_class(1025, WIDE, 2000, F32) == VC_BLOCK_SEARCH);
    CHECK(val_class(1024, WIDE, 2000, F64) == VC_BLOCK_SEARCH);  // (FP64: 682)
    // ---- block-direct: span <= 39,936 (156 KiB of FP32 sums beside the stage)
    CHECK(val_class(3000, 39935, 4000, F32) == VC_BLOCK_DIRECT);
    CHECK(val_class(3000, 39936, 4000, F32) == VC_BLOCK_DIRECT);
    CHECK(val_class(3000, 39937, 4000, F32) == VC_BLOCK_SEARCH);
    CHECK(val_class(3000, 39936, 4000, F64) == VC_BLOCK_SEARCH);  // (FP64: 19,968)
    // ---- block-search: n <= 19,968; past it the global class
    CHECK(val_class(19967, WIDE, 20000, F32) == VC_BLOCK_SEARCH);
    CHECK(val_class(19968, WIDE, 20000, F32) == VC_BLOCK_SEARCH);
    CHECK(val_class(19969, WIDE, 20000, F32) == VC_GLOBAL);
    CHECK(val_class(19968, WIDE, 20000, F64) == VC_GLOBAL);  // (FP64: 13,312)
    // ---- the edges that are counts, not bytes, stay: team n and products, the wave product cap, the dense ratio
    CHECK(val_class(0, 0, 100, F32) == VC_NONE);
    CHECK(val_class(63, 100, 10, F32) == VC_TEAM && val_class(64, 100, 10, F32) == VC_TEAM);
    CHECK(val_class(65, 100, 10, F32) == VC_WAVE_DIRECT);
    CHECK(val_class(10, 50, 511, F32) == VC_TEAM && val_class(10, 50, 512, F32) == VC_TEAM);
    CHECK(val_class(10, 50, 513, F32) == VC_WAVE_DIRECT);
    CHECK(val_class(10, WIDE, 512, F32) == VC_TEAM && val_class(10, WIDE, 513, F32) == VC_WAVE_SEARCH);
    CHECK(val_class(64, 100, 0, F32) == VC_TEAM && val_class(65, 100, 0, F32) == VC_GLOBAL);
    CHECK(val_class(100, 500, 2047, F32) == VC_WAVE_DIRECT && val_class(100, 500, 2048, F32) == VC_WAVE_DIRECT);
    CHECK(val_class(100, 500, 2049, F32) == VC_BLOCK_DIRECT);
    CHECK(val_class(100, WIDE, 2048, F32) == VC_WAVE_SEARCH && val_class(100, WIDE, 2049, F32) == VC_BLOCK_SEARCH);
    CHECK(val_class(200, 3199, 1000, F32) == VC_BLOCK_DIRECT);  // span <= 16 n: a block's direct table before a wave searches
    CHECK(val_class(200, 3200, 1000, F32) == VC_BLOCK_DIRECT);
    CHECK(val_class(200, 3201, 1000, F32) == VC_WAVE_SEARCH);
    // the rows of the test zoo one FP64 workgroup cannot hold: both fit an FP32 one
    CHECK(val_class(21120, 21120, 21120, F32) == VC_BLOCK_DIRECT);  // 4 B x 21120 = 84,480
    CHECK(val_class(20000, 1900000, 20000, F32) == VC_GLOBAL);      // 8 B x 20000 = 160,000 > 159,744

    // ---- vb = 8 is what the old signatures return
    for (int n : {0, 1, 63, 64, 65, 100, 681, 682, 683, 1024, 1025, 3000, 13312, 13313, 19968, 19969, 30000})
        for (long long span : {1LL, 100LL, 1023LL, 1024LL, 1025LL, 2048LL, 2049LL, 19968LL, 19969LL, 39936LL, 39937LL, WIDE})
            for (long long prod : {0LL, 1LL, 512LL, 513LL, 2048LL, 2049LL, 100000LL}) {
                const int cls = val_class(n, span, prod);
                CHECK(val_class(n, span, prod, F64) == cls);
                CHECK(val_row_need(cls, n, span, F64) == val_row_need(cls, n, span));
                for (int form : {VM_AUTO, VM_PRODUCT, VM_DOT})
                    for (long long cost : {0LL, 10LL, 100000LL}) {
                        CHECK(val_class_masked(n, span, prod, 3, cost, form, VAL_DOT_RATIO, F64) ==
                              val_class_masked(n, span, prod, 3, cost, form));
                        // the dot class is chosen by counts: the same rows take it in FP32
                        const int m4 = val_class_masked(n, span, prod, 3, cost, form, VAL_DOT_RATIO, F32);
                        CHECK((m4 == VC_DOT) == (val_class_masked(n, span, prod, 3, cost, form) == VC_DOT));
                        if (m4 != VC_DOT) CHECK(m4 == val_class(n, span, prod, F32));
                    }
            }
    for (int c = 0; c < VAL_NCLASS; ++c) CHECK(val_class_cap(c, F64) == val_class_cap(c));
    CHECK(val_lds_search(65, F64) == val_lds_search(65) && val_lds_direct(1000, F64) == val_lds_direct(1000));

    // ---- LDS needs and caps, FP32
    CHECK(val_lds_search(63, F32) == 512 && val_lds_search(64, F32) == 512 && val_lds_search(65, F32) == 528);
    CHECK(val_lds_direct(2048, F32) == 8192 && val_lds_search(1024, F32) == 8192);
    CHECK(val_lds_direct(39936, F32) == 159744 && val_lds_search(19968, F32) == 159744);
    CHECK(val_row_need(VC_TEAM, 5, 999, F32) == 48 && val_row_need(VC_WAVE_DIRECT, 5, 999, F32) == 3996 &&
          val_row_need(VC_WAVE_SEARCH, 101, 999, F32) == 816 && val_row_need(VC_BLOCK_DIRECT, 5, 30000, F32) == 120000 &&
          val_row_need(VC_BLOCK_SEARCH, 1001, 5, F32) == 8016 && val_row_need(VC_GLOBAL, 5, 5, F32) == 0 &&
          val_row_need(VC_DOT, 5, 5, F32) == 0 && val_row_need(VC_NONE, 0, 0, F32) == 0);
    CHECK(val_class_cap(VC_TEAM, F32) == 512 && val_class_cap(VC_WAVE_DIRECT, F32) == 8192 &&
          val_class_cap(VC_WAVE_SEARCH, F32) == 8192 && val_class_cap(VC_BLOCK_DIRECT, F32) == 159744 &&
          val_class_cap(VC_BLOCK_SEARCH, F32) == 159744 && val_class_cap(VC_GLOBAL, F32) == 0 && val_class_cap(VC_DOT, F32) == 0);
    // every row fits what its class may declare, and passes the guard of a slice of exactly its need
    for (int vb : {F32, F64})
        for (int n = 1; n <= 21000; n += 7)
            for (long long span : {(long long)n, 2LL * n, 17LL * n, 2048LL, 2049LL, 39936LL, 39937LL, WIDE})
                for (long long prod : {0LL, 1LL, 512LL, 513LL, 2048LL, 2049LL}) {
                    if (span < n) continue;
                    const int cls = val_class(n, span, prod, vb);
                    CHECK(cls > VC_NONE && cls < VC_COUNT);
                    const int need = val_row_need(cls, n, span, vb);
                    CHECK(need <= val_class_cap(cls, vb));
                    if (cls == VC_WAVE_DIRECT || cls == VC_BLOCK_DIRECT) {
                        CHECK(val_slice_fits(span, need, vb) && !val_slice_fits(span, need - 1, vb));
                    } else if (cls != VC_GLOBAL) {
                        CHECK(n <= val_slice_entries(need, vb));
                    }
                }

    // ---- the slice guards at (region, vb): entries held, and fits / does not fit at the exact byte
    CHECK(val_slice_entries(8192, F32) == 1024 && val_slice_entries(8191, F32) == 1023 && val_slice_entries(8200, F32) == 1025);
    CHECK(val_slice_entries(8192, F64) == 682 && val_slice_entries(8184, F64) == 682 && val_slice_entries(8183, F64) == 681);
    CHECK(val_slice_entries(512, F32) == 64 && val_slice_entries(511, F32) == 63 && val_slice_entries(768, F64) == 64 &&
          val_slice_entries(767, F64) == 63);
    CHECK(val_slice_entries(159744, F32) == 19968 && val_slice_entries(159744, F64) == 13312);
    CHECK(val_slice_entries(0, F32) == 0 && val_slice_entries(7, F32) == 0 && val_slice_entries(11, F64) == 0);
    // (sums and columns of the entries held stay inside the region)
    for (int region : {16, 48, 512, 768, 1280, 8192, 32768, 159744})
        for (int vb : {F32, F64}) CHECK((long long)val_slice_entries(region, vb) * (vb + 4) <= region);
    CHECK(val_slice_fits(2048, 8192, F32) && !val_slice_fits(2049, 8192, F32) && !val_slice_fits(2048, 8191, F32));
    CHECK(val_slice_fits(1024, 8192, F64) && !val_slice_fits(1025, 8192, F64) && !val_slice_fits(1024, 8191, F64));
    CHECK(val_slice_fits(39936, 159744, F32) && !val_slice_fits(39937, 159744, F32));
    CHECK(val_slice_fits(19968, 159744, F64) && !val_slice_fits(19969, 159744, F64));
    CHECK(val_slice_fits(1, 4, F32) && !val_slice_fits(1, 3, F32) && val_slice_fits(1, 8, F64) && !val_slice_fits(1, 7, F64));
    CHECK(!val_slice_fits(0, 8192, F32) && !val_slice_fits(-5, 8192, F32) && !val_slice_fits(1, 0, F32));
    CHECK(!val_slice_fits(0x7fffffffffffLL, 8192, F32));  // (no overflow: the span is not multiplied)
    // an FP64 guard on an FP32 launch would skip rows that fit; an FP32 guard on an FP64 launch would overrun
    CHECK(val_slice_fits(2048, 8192, F32) != val_slice_fits(2048, 8192, F64));
    CHECK(val_slice_entries(8192, F32) != val_slice_entries(8192, F64));

    // ---- plan_values at vb = 4
    CHECK(plan_values(ValCounts{}, F32).n == 0);
    {
        const ValPlan p = plan_values(one(VC_TEAM, 1, 512), F32);
        CHECK(p.n == 1 && p.launch[0].kernel == VK_TEAM && p.launch[0].cls == VC_TEAM && p.launch[0].grid == 1 &&
              p.launch[0].block == 256 && p.launch[0].region == 512 && p.launch[0].lds == 16384 && p.launch[0].count == 1);
        const ValPlan q = plan_values(one(VC_TEAM, 33, 48), F32);  // n 5 or 6: 8 B x 6
        CHECK(q.n == 1 && q.launch[0].grid == 2 && q.launch[0].region == 48 && q.launch[0].lds == 1536);
        const ValPlan r = plan_values(one(VC_TEAM, 33, 72), F32);  // (not an FP32 need: rounded up to whole entry pairs)
        CHECK(r.launch[0].region == 80 && r.launch[0].lds == 2560);
        const ValPlan z = plan_values(one(VC_TEAM, 33, 0), F32);  // no need counted: the cap
        CHECK(z.launch[0].region == 512);
        CHECK(plan_values(one(VC_TEAM, 1, 768), F64).launch[0].lds == 24576);  // FP64 as before
    }
    {
        const ValPlan p = plan_values(one(VC_WAVE_DIRECT, 1, 1200), F32);  // span 300
        CHECK(p.n == 1 && p.launch[0].kernel == VK_WAVE_DIRECT && p.launch[0].grid == 1 && p.launch[0].block == 256 &&
              p.launch[0].region == 1280 && p.launch[0].lds == 5120);
        const ValPlan q = plan_values(one(VC_WAVE_DIRECT, 5, 8192), F32);  // span 2048
        CHECK(q.n == 1 && q.launch[0].grid == 2 && q.launch[0].region == 8192 && q.launch[0].lds == 32768);
    }
    {
        const ValPlan p = plan_values(one(VC_WAVE_SEARCH, 1, 800), F32);  // n 100
        CHECK(p.n == 1 && p.launch[0].kernel == VK_WAVE_SEARCH && p.launch[0].grid == 1 && p.launch[0].block == 256 &&
              p.launch[0].region == 1024 && p.launch[0].lds == 4096);
        const ValPlan q = plan_values(one(VC_WAVE_SEARCH, 9, 8192), F32);  // n 1024
        CHECK(q.launch[0].grid == 3 && q.launch[0].region == 8192 && q.launch[0].lds == 32768);
    }
    {
        const ValPlan p = plan_values(one(VC_BLOCK_DIRECT, 1, 8196), F32);  // span 2049
        CHECK(p.n == 1 && p.launch[0].kernel == VK_BLOCK_DIRECT && p.launch[0].grid == 1 && p.launch[0].block == 256 &&
              p.launch[0].lds == 10240 && p.launch[0].region == 10240);
        CHECK(plan_values(one(VC_BLOCK_DIRECT, 1, 32768), F32).launch[0].block == 256);  // span 8192
        const ValPlan q = plan_values(one(VC_BLOCK_DIRECT, 1, 32772), F32);               // span 8193
        CHECK(q.launch[0].block == 1024 && q.launch[0].lds == 34816);
        const ValPlan r = plan_values(one(VC_BLOCK_DIRECT, 1, 159744), F32);  // span 39,936
        CHECK(r.launch[0].block == 1024 && r.launch[0].lds == 159744 && r.launch[0].region == 159744);
    }
    {
        const ValPlan p = plan_values(one(VC_BLOCK_SEARCH, 1, 159744), F32);  // n 19,968
        CHECK(p.n == 1 && p.launch[0].kernel == VK_BLOCK_SEARCH && p.launch[0].grid == 1 && p.launch[0].block == 1024 &&
              p.launch[0].lds == 159744);
        const ValPlan q = plan_values(one(VC_BLOCK_SEARCH, 3, 8208), F32);  // n 1025 or 1026
        CHECK(q.launch[0].grid == 3 && q.launch[0].block == 256 && q.launch[0].lds == 10240);
    }
    {
        const ValPlan p = plan_values(one(VC_GLOBAL, 1, 0), F32);
        CHECK(p.n == 1 && p.launch[0].kernel == VK_GLOBAL && p.launch[0].grid == 1 && p.launch[0].block == 1024 &&
              p.launch[0].lds == 0);
        const ValPlan d = plan_values(one(VC_DOT, 9, 0), F32);
        CHECK(d.n == 1 && d.launch[0].kernel == VK_DOT && d.launch[0].cls == VC_DOT && d.launch[0].grid == 3 &&
              d.launch[0].block == 256 && d.launch[0].lds == 0);
    }
    // every class at once, every need: no launch above 163,840 B static + dynamic, block launches of at most
    // 32 KiB on 256 threads and of more on 1024, regions that hold the need; plan_grad: the same launches, the dot
    // rows on the global-form kernel
    for (int vb : {F32, F64})
        for (int need : {0, 16, 48, 512, 800, 1200, 8192, 8196, 32768, 32772, 100000, 159744}) {
            ValCounts c{};
            for (int k = VC_TEAM; k < VAL_NCLASS; ++k) {
                c.rows[k] = 10 * (k + 1);
                c.need[k] = need < val_class_cap(k, vb) ? need : val_class_cap(k, vb);
            }
            const ValPlan p = plan_values(c, vb), g = plan_grad(c, vb);
            CHECK(p.n == 7 && g.n == 7);
            const int order[7] = {VC_DOT, VC_GLOBAL, VC_BLOCK_SEARCH, VC_BLOCK_DIRECT, VC_WAVE_SEARCH, VC_WAVE_DIRECT, VC_TEAM};
            for (int i = 0; i < 7 && i < p.n; ++i) {
                const ValLaunch& l = p.launch[i];
                CHECK(l.cls == order[i] && l.count == c.rows[order[i]]);
                CHECK(l.lds >= 0 && l.lds + VAL_STAGE_BYTES <= 163840);
                CHECK(l.region >= c.need[l.cls] && l.region <= val_class_cap(l.cls, vb));
                if (l.cls == VC_BLOCK_DIRECT || l.cls == VC_BLOCK_SEARCH) {
                    CHECK(l.lds == l.region && (l.block == 256) == (l.lds <= 32768) && (l.block == 1024) == (l.lds > 32768));
                } else if (l.cls == VC_WAVE_DIRECT || l.cls == VC_WAVE_SEARCH) {
                    CHECK(l.block == 256 && l.lds == 4 * l.region && l.lds <= 32768);
                } else if (l.cls == VC_TEAM) {
                    CHECK(l.block == 256 && l.lds == 32 * l.region && l.lds <= (vb == F32 ? 16384 : 24576));
                    CHECK(l.region % (2 * (vb + 4)) == 0);
                }
                ValLaunch want = l;
                if (l.kernel == VK_DOT) want.kernel = VK_GLOBAL;
                CHECK(same_launch(g.launch[i], want));
            }
        }
    {   // plan_grad at vb = 4 against literals
        ValCounts c = one(VC_TEAM, 40, 512);
        c.rows[VC_DOT] = 9;
        c.rows[VC_WAVE_SEARCH] = 2;
        c.need[VC_WAVE_SEARCH] = 8192;
        const ValPlan g = plan_grad(c, F32);
        CHECK(g.n == 3);
        CHECK(g.launch[0].kernel == VK_GLOBAL && g.launch[0].cls == VC_DOT && g.launch[0].grid == 3 && g.launch[0].block == 256 &&
              g.launch[0].lds == 0 && g.launch[0].count == 9);
        CHECK(g.launch[1].kernel == VK_WAVE_SEARCH && g.launch[1].grid == 1 && g.launch[1].block == 256 &&
              g.launch[1].region == 8192 && g.launch[1].lds == 32768 && g.launch[1].count == 2);
        CHECK(g.launch[2].kernel == VK_TEAM && g.launch[2].grid == 2 && g.launch[2].block == 256 && g.launch[2].region == 512 &&
              g.launch[2].lds == 16384 && g.launch[2].count == 40);
    }
    // the defaulted argument is FP64
    {
        ValCounts c{};
        for (int k = VC_TEAM; k < VAL_NCLASS; ++k) {
            c.rows[k] = 7 * k;
            c.need[k] = val_class_cap(k) / 2;
        }
        const ValPlan a = plan_values(c), b = plan_values(c, F64), ga = plan_grad(c), gb = plan_grad(c, F64);
        CHECK(a.n == b.n && ga.n == gb.n);
        for (int i = 0; i < a.n; ++i) CHECK(same_launch(a.launch[i], b.launch[i]) && same_launch(ga.launch[i], gb.launch[i]));
    }

    if (failures) return 1;
    std::printf("valplan f32 ok\n");
    return 0;
}
