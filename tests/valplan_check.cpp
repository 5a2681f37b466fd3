// valplan_check.cpp -- the values-only row classes and launch plan (csrc/mhs_valplan.hpp) on the host:
// the class of rows one below, at and one above every threshold on the n, span and product axes,
// each class's LDS need, and plan_values' launches, against hand-computed literals; and the layout of
// plan creation's counter block and status words (fields inside the block, disjoint, 64-bit counts aligned).
// Built by tests/test_values_host.py with -fsanitize=address,undefined; prints "valplan ok".
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

int main() {
    const long long WIDE = 1000000;  // a span no direct class holds
    // class ids are part of the ABI (mhs_values_info::rows)
    CHECK(VC_NONE == 0 && VC_TEAM == 1 && VC_WAVE_DIRECT == 2 && VC_WAVE_SEARCH == 3 && VC_BLOCK_DIRECT == 4 &&
          VC_BLOCK_SEARCH == 5 && VC_GLOBAL == 6 && VAL_NCLASS == 8);

    // ---- n == 0, and rows without products
    CHECK(val_class(0, 0, 0) == VC_NONE);
    CHECK(val_class(0, 0, 100) == VC_NONE);
    CHECK(val_class(1, 1, 0) == VC_TEAM);
    CHECK(val_class(64, 100, 0) == VC_TEAM);      // short: the team zero-fills
    CHECK(val_class(65, 100, 0) == VC_GLOBAL);    // longer: zero fill without LDS
    CHECK(val_class(65, 100, 1) == VC_WAVE_DIRECT);

    // ---- team: n <= 64 and products <= 512
    CHECK(val_class(63, 100, 10) == VC_TEAM);
    CHECK(val_class(64, 100, 10) == VC_TEAM);
    CHECK(val_class(65, 100, 10) == VC_WAVE_DIRECT);
    CHECK(val_class(10, 50, 511) == VC_TEAM);
    CHECK(val_class(10, 50, 512) == VC_TEAM);
    CHECK(val_class(10, 50, 513) == VC_WAVE_DIRECT);
    CHECK(val_class(10, WIDE, 512) == VC_TEAM);   // the team searches: span does not matter
    CHECK(val_class(10, WIDE, 513) == VC_WAVE_SEARCH);

    // ---- wave-direct: span <= 1024 (8 KiB of FP64 sums)
    CHECK(val_class(100, 1023, 1000) == VC_WAVE_DIRECT);
    CHECK(val_class(100, 1024, 1000) == VC_WAVE_DIRECT);
    CHECK(val_class(100, 1025, 1000) == VC_BLOCK_DIRECT);  // 1025 <= 16 * 100: dense enough for a block
    // ---- the dense ratio: span <= 16 n goes to a block's direct table before a wave searches
    CHECK(val_class(70, 1119, 1000) == VC_BLOCK_DIRECT);
    CHECK(val_class(70, 1120, 1000) == VC_BLOCK_DIRECT);
    CHECK(val_class(70, 1121, 1000) == VC_WAVE_SEARCH);
    // ---- wave-search: n <= 682 (12 B per entry in 8 KiB)
    CHECK(val_class(681, WIDE, 1000) == VC_WAVE_SEARCH);
    CHECK(val_class(682, WIDE, 1000) == VC_WAVE_SEARCH);
    CHECK(val_class(683, WIDE, 1000) == VC_BLOCK_SEARCH);
    // ---- wave classes: products <= 2048
    CHECK(val_class(100, 500, 2047) == VC_WAVE_DIRECT);
    CHECK(val_class(100, 500, 2048) == VC_WAVE_DIRECT);
    CHECK(val_class(100, 500, 2049) == VC_BLOCK_DIRECT);
    CHECK(val_class(100, WIDE, 2048) == VC_WAVE_SEARCH);
    CHECK(val_class(100, WIDE, 2049) == VC_BLOCK_SEARCH);
    // ---- block-direct: span <= 19968 (156 KiB of FP64 sums beside the 4 KiB stage), also for sparse rows a wave cannot search
    CHECK(val_class(700, 19967, 1000) == VC_BLOCK_DIRECT);
    CHECK(val_class(700, 19968, 1000) == VC_BLOCK_DIRECT);
    CHECK(val_class(700, 19969, 1000) == VC_BLOCK_SEARCH);
    // ---- block-search: n <= 13312; past it the global class
    CHECK(val_class(13311, WIDE, 100000) == VC_BLOCK_SEARCH);
    CHECK(val_class(13312, WIDE, 100000) == VC_BLOCK_SEARCH);
    CHECK(val_class(13313, WIDE, 100000) == VC_GLOBAL);
    // the rows of the test zoo that one workgroup cannot hold
    CHECK(val_class(21120, 21120, 21120) == VC_GLOBAL);   // contiguous: 8 B x 21120 = 168,960 > 159,744
    CHECK(val_class(20000, 1900000, 20000) == VC_GLOBAL); // scattered: 12 B x 20000 = 240,000
    CHECK(val_class(64, 64, 192000) == VC_BLOCK_DIRECT);  // 3000 duplicates of one B row: a block's work

    // ---- LDS needs
    CHECK(val_lds_search(63) == 768 && val_lds_search(64) == 768 && val_lds_search(65) == 792);
    CHECK(val_lds_direct(1024) == 8192 && val_lds_search(682) == 8184);
    CHECK(val_lds_direct(19968) == 159744 && val_lds_search(13312) == 159744);
    CHECK(val_row_need(VC_TEAM, 5, 999) == 72 && val_row_need(VC_WAVE_DIRECT, 5, 999) == 7992 &&
          val_row_need(VC_BLOCK_SEARCH, 1001, 5) == 12024 && val_row_need(VC_GLOBAL, 5, 5) == 0 &&
          val_row_need(VC_NONE, 0, 0) == 0);
    CHECK(val_class_cap(VC_TEAM) == 768 && val_class_cap(VC_WAVE_DIRECT) == 8192 && val_class_cap(VC_WAVE_SEARCH) == 8192 &&
          val_class_cap(VC_BLOCK_DIRECT) == 159744 && val_class_cap(VC_BLOCK_SEARCH) == 159744 &&
          val_class_cap(VC_GLOBAL) == 0);
    for (int c = 0; c < VC_COUNT; ++c) CHECK(val_class_cap(c) + VAL_STAGE_BYTES <= 163840);  // static stage + dynamic
    CHECK(VAL_STAGE_BYTES == 4096);
    // every row fits what its class may declare
    for (int n = 1; n <= 14000; n += 7)
        for (long long span : {(long long)n, 2LL * n, 17LL * n, 19968LL, 19969LL, WIDE})
            for (long long prod : {0LL, 1LL, 512LL, 513LL, 2048LL, 2049LL}) {
                if (span < n) continue;
                const int cls = val_class(n, span, prod);
                CHECK(cls > VC_NONE && cls < VC_COUNT);
                CHECK(val_row_need(cls, n, span) <= val_class_cap(cls));
            }

    // ---- plan_values
    {
        const ValCounts z{};
        CHECK(plan_values(z).n == 0);
    }
    {
        const ValPlan p = plan_values(one(VC_TEAM, 1, 768));
        CHECK(p.n == 1 && p.launch[0].kernel == VK_TEAM && p.launch[0].cls == VC_TEAM && p.launch[0].grid == 1 &&
              p.launch[0].block == 256 && p.launch[0].region == 768 && p.launch[0].lds == 24576 && p.launch[0].count == 1);
        const ValPlan q = plan_values(one(VC_TEAM, 33, 72));
        CHECK(q.n == 1 && q.launch[0].grid == 2 && q.launch[0].region == 72 && q.launch[0].lds == 2304);
    }
    {
        const ValPlan p = plan_values(one(VC_WAVE_DIRECT, 1, 2400));  // span 300
        CHECK(p.n == 1 && p.launch[0].kernel == VK_WAVE_DIRECT && p.launch[0].grid == 1 && p.launch[0].block == 256 &&
              p.launch[0].region == 2560 && p.launch[0].lds == 10240);
        const ValPlan q = plan_values(one(VC_WAVE_DIRECT, 5, 8192));
        CHECK(q.n == 1 && q.launch[0].grid == 2 && q.launch[0].region == 8192 && q.launch[0].lds == 32768);
    }
    {
        const ValPlan p = plan_values(one(VC_WAVE_SEARCH, 1, 1200));  // n 100
        CHECK(p.n == 1 && p.launch[0].kernel == VK_WAVE_SEARCH && p.launch[0].grid == 1 && p.launch[0].block == 256 &&
              p.launch[0].region == 1280 && p.launch[0].lds == 5120);
    }
    {
        const ValPlan p = plan_values(one(VC_BLOCK_DIRECT, 1, 8800));  // span 1100
        CHECK(p.n == 1 && p.launch[0].kernel == VK_BLOCK_DIRECT && p.launch[0].grid == 1 && p.launch[0].block == 256 &&
              p.launch[0].lds == 10240 && p.launch[0].region == 10240);
        CHECK(plan_values(one(VC_BLOCK_DIRECT, 1, 32768)).launch[0].block == 256);
        const ValPlan q = plan_values(one(VC_BLOCK_DIRECT, 1, 32769));
        CHECK(q.launch[0].block == 1024 && q.launch[0].lds == 34816);
        const ValPlan r = plan_values(one(VC_BLOCK_DIRECT, 1, 159744));
        CHECK(r.launch[0].block == 1024 && r.launch[0].lds == 159744);
    }
    {
        const ValPlan p = plan_values(one(VC_BLOCK_SEARCH, 1, 159744));
        CHECK(p.n == 1 && p.launch[0].kernel == VK_BLOCK_SEARCH && p.launch[0].grid == 1 && p.launch[0].block == 1024 &&
              p.launch[0].lds == 159744);
        const ValPlan q = plan_values(one(VC_BLOCK_SEARCH, 3, 12000));
        CHECK(q.launch[0].grid == 3 && q.launch[0].block == 256 && q.launch[0].lds == 12288);
    }
    {
        const ValPlan p = plan_values(one(VC_GLOBAL, 1, 0));
        CHECK(p.n == 1 && p.launch[0].kernel == VK_GLOBAL && p.launch[0].grid == 1 && p.launch[0].block == 1024 &&
              p.launch[0].lds == 0);
    }
    {   // every class at once: heaviest rows first, one launch each, class 0 none
        ValCounts c{};
        for (int k = 0; k < VC_COUNT; ++k) {
            c.rows[k] = 10 * (k + 1);
            c.need[k] = val_class_cap(k);
        }
        const ValPlan p = plan_values(c);
        CHECK(p.n == 6);
        const int order[6] = {VC_GLOBAL, VC_BLOCK_SEARCH, VC_BLOCK_DIRECT, VC_WAVE_SEARCH, VC_WAVE_DIRECT, VC_TEAM};
        for (int i = 0; i < 6 && i < p.n; ++i) {
            CHECK(p.launch[i].cls == order[i] && p.launch[i].count == c.rows[order[i]]);
            CHECK(p.launch[i].lds + VAL_STAGE_BYTES <= 163840);
        }
    }
    // grids: at least one block, never more blocks than rows, capped
    for (int cls = VC_TEAM; cls < VC_COUNT; ++cls)
        for (int rows : {1, 2, 3, 4, 5, 31, 32, 33, 1000, 70000, 5000000}) {
            const ValPlan p = plan_values(one(cls, rows, val_class_cap(cls)));
            CHECK(p.n == 1);
            CHECK(p.launch[0].grid >= 1 && p.launch[0].grid <= rows && p.launch[0].grid <= 16384);
            CHECK(p.launch[0].lds + VAL_STAGE_BYTES <= 163840 && p.launch[0].count == rows);
        }
    CHECK(plan_values(one(VC_TEAM, 5000000, 768)).launch[0].grid == 16384);
    CHECK(plan_values(one(VC_WAVE_SEARCH, 1000, 8184)).launch[0].grid == 250);
    CHECK(plan_values(one(VC_BLOCK_DIRECT, 70000, 8800)).launch[0].grid == 4096);
    CHECK(plan_values(one(VC_BLOCK_SEARCH, 39, 8800)).launch[0].grid == 39);  // a block per hub row
    CHECK(plan_values(one(VC_GLOBAL, 70000, 0)).launch[0].grid == 1024);

    // ---- the counter block of plan creation: every field inside VAL_CNT_INTS, no two overlapping (the 32-bit
    // counters one int, the two 64-bit counts two), the 64-bit counts on 8-byte boundaries
    {
        struct Field {
            int at, ints;
        };
        Field f[3 * VAL_NCLASS + 2];
        int nf = 0;
        for (int c = 0; c < VAL_NCLASS; ++c) {
            f[nf++] = {val_cnt_rows(c), 1};
            f[nf++] = {val_cnt_cursor(c), 1};
            f[nf++] = {val_cnt_need(c), 1};
        }
        f[nf++] = {VAL_CNT_PRODUCTS, 2};
        f[nf++] = {VAL_CNT_KEPT, 2};
        CHECK(nf == 3 * VAL_NCLASS + 2);
        for (int i = 0; i < nf; ++i) {
            CHECK(f[i].at >= 0 && f[i].at + f[i].ints <= VAL_CNT_INTS);
            for (int j = 0; j < i; ++j) CHECK(f[i].at + f[i].ints <= f[j].at || f[j].at + f[j].ints <= f[i].at);
        }
        CHECK(VAL_CNT_PRODUCTS % 2 == 0 && VAL_CNT_KEPT % 2 == 0);
        CHECK(val_cnt_rows(0) == 0 && val_cnt_rows(1) == BINCNT_STRIDE);  // one counter per stride
        // the status words: one per check, inside VAL_STATUS_INTS, which is whole 8-byte words
        CHECK(VS_APTR == 0 && VS_BPTR == 1 && VS_CPTR == 2 && VS_ACOL == 3 && VS_CCOL == 4 && VS_PRODUCTS == 5 &&
              VS_BCOL == 6 && VS_COUNT == 7);
        CHECK(VS_COUNT <= VAL_STATUS_INTS && VAL_STATUS_INTS % 2 == 0 && VAL_STATUS_INTS == 8);
    }

    if (failures) return 1;
    std::printf("valplan ok\n");
    return 0;
}
