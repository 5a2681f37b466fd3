// Host check of plan_numeric (mh-spgemm_amd/csrc/mhs_numplan.hpp), the numeric launch plan as a
// function of the Stats a call publishes: a stand-alone program, built with
// -fsanitize=address,undefined by tests/test_host.py.  Every expected figure below is a literal
// worked out by hand from the bins' rules (the arithmetic is in the comments), none comes from the
// helpers under test.
#include "../mh-spgemm_amd/csrc/mhs_numplan.hpp"

#include <cstdio>
#include <cstring>

using namespace mhs;

static int failures = 0;
#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            ++failures;                                                 \
            fprintf(stderr, "line %d: %s\n", __LINE__, #cond);          \
        }                                                               \
    } while (0)

static bool same(const NumPlan& a, const NumPlan& b) { return memcmp(&a, &b, sizeof(NumPlan)) == 0; }

// one expected launch: the fields every kind has
struct Want {
    int kernel, variant, grid, block, lds, list_bin, list_off, count, slot, after_split;
};
static void check_launch(const NumLaunch& l, const Want& w, int line) {
    const bool ok = l.kernel == w.kernel && l.variant == w.variant && l.grid == w.grid && l.block == w.block &&
                    l.lds == w.lds && l.list_bin == w.list_bin && l.list_off == w.list_off && l.count == w.count &&
                    l.slot == w.slot && l.after_split == w.after_split;
    if (!ok) {
        ++failures;
        fprintf(stderr, "line %d: launch {k %d v %d grid %d block %d lds %d bin %d off %d count %d slot %d split %d}\n",
                line, l.kernel, l.variant, l.grid, l.block, l.lds, l.list_bin, l.list_off, l.count, l.slot,
                l.after_split);
    }
}
#define LAUNCH(l, ...) check_launch(l, Want{__VA_ARGS__}, __LINE__)

// Bins: WS 1, W16 2, B256 3, B1024 4, GLOBAL 5, WSG 6, W16G 7, tiny classes 0..5 at 8..13, WSH 14,
// W16H 15.  Every bin non-empty: bin b holds 1000 + b rows.
static Stats every_bin() {
    Stats h{};
    h.flop = 1ull << 30;
    h.nnzC = 1 << 20;
    for (int b = 1; b < 16; ++b) h.num_count[b] = 1000 + b;
    h.num_block_big[0] = 3;
    h.num_block_big[1] = 2;
    h.num_block_need[0] = 40000;
    h.num_block_need[1] = 120000;
    h.num_block_small_need[0] = 9000;
    h.num_block_small_need[1] = 30000;
    h.num_wave_need[0] = 3000;
    h.num_wave_need[1] = 9000;
    h.num_global_need = 500000;
    return h;
}
static NumShape shape(int M, bool slot_rows, bool split) { return NumShape{M, 1000, 1000, 0, slot_rows, split, 128}; }

// Every non-empty bin's rows in exactly one launch (split parts summing to the bin), no launch
// past the LDS of a workgroup or with an empty grid.
static void check_rows(const NumPlan& p, const Stats& h) {
    int rows[16] = {};
    for (int i = 0; i < p.n; ++i) {
        const NumLaunch& l = p.launch[i];
        CHECK(l.grid > 0 && l.block > 0 && l.lds >= 0 && l.lds <= 163840 && l.count > 0);
        if (l.list_bin > 0) rows[l.list_bin] += l.count;
        else if (l.list_bin == LIST_SPLIT) rows[l.kernel == NK_BLOCK1024 ? 4 : 3] += l.count;
        if (l.list_bin == LIST_CLASSES || l.kernel == NK_COPY_HASH)
            for (int k = 0; k < l.fused.nclass; ++k) rows[8 + l.fused.c[k]] += l.fused.count[k];
    }
    for (int b = 1; b < 16; ++b) CHECK(rows[b] == (h.num_count[b] > 0 ? h.num_count[b] : 0));
}

static void test_every_bin() {
    const Stats h = every_bin();
    const NumPlan p = plan_numeric(h, shape(100000, false, true));
    CHECK(p.n == 14 && p.o32 == 1);
    const NumLaunch* l = p.launch;
    // block headers: 256 threads 1024 + 4 * 65 * 16 = 5184, 1024 threads 1024 + 12 * 65 * 16 = 13504
    // global: min(1005, 128) blocks, the 1024-thread header alone, scratch 500000 (a multiple of 16)
    LAUNCH(l[0], NK_GLOBAL, 0, 128, 1024, 13504, 5, 0, 1005, 5, 0);
    CHECK(l[0].gbytes == 500000);
    // B1024: its part of split_list first: 1002 small rows at 0, the 2 hub rows at 1002.
    // LDS (13504 + 120000 + 2047) & ~2047 = 66 * 2048; (13504 + 30000 + 2047) & ~2047 = 22 * 2048
    LAUNCH(l[1], NK_BLOCK1024, 0, 8, 1024, 135168, LIST_SPLIT, 1002, 2, 29, 1);
    LAUNCH(l[2], NK_BLOCK1024, 0, 256, 1024, 45056, LIST_SPLIT, 0, 1002, 4, 1);
    // B256 after B1024's 1004 rows: 1000 small rows at 1004, the 3 hub rows at 2004.
    // LDS (5184 + 40000 + 2047) & ~2047 = 23 * 2048; (5184 + 9000 + 2047) & ~2047 = 7 * 2048
    LAUNCH(l[3], NK_BLOCK256, 0, 8, 256, 47104, LIST_SPLIT, 2004, 3, 28, 1);
    LAUNCH(l[4], NK_BLOCK256, 0, 1000, 256, 14336, LIST_SPLIT, 1004, 1000, 3, 1);
    // wave bins: 4 rows a block, grids rounded up to 8: ceil(1015 / 4) = 254 -> 256
    LAUNCH(l[5], NK_HASH16, 0, 256, 256, 40960, 15, 0, 1015, 15, 0);
    CHECK(l[5].qall == 1);
    LAUNCH(l[6], NK_HASH, 0, 256, 256, 20480, 14, 0, 1014, 14, 0);
    LAUNCH(l[7], NK_DIRECT16, 0, 256, 256, 40960, 2, 0, 1002, 2, 0);
    // 64-lane tiny classes: 4 rows a block, LDS 256 * K * 8 (K = 8, 4)
    LAUNCH(l[8], NK_TINY64, 5, 256, 256, 16384, 13, 0, 1013, 13, 0);
    LAUNCH(l[9], NK_TINY64, 4, 256, 256, 8192, 12, 0, 1012, 12, 0);
    // classes 3..0 in one launch: 8 / 16 / 32 / 64 rows a block: ceil(1011 / 8) = 127 -> 128,
    // ceil(1010 / 16) = 64, ceil(1009 / 32) = 32, ceil(1008 / 64) = 16
    LAUNCH(l[10], NK_TINY_SMALL, 0, 240, 256, 8192, LIST_CLASSES, 0, 4038, 0, 0);
    const TinyFused& f = l[10].fused;
    CHECK(f.nclass == 4 && f.c[0] == 3 && f.c[1] == 2 && f.c[2] == 1 && f.c[3] == 0);
    CHECK(f.count[0] == 1011 && f.count[1] == 1010 && f.count[2] == 1009 && f.count[3] == 1008);
    CHECK(f.blk0[0] == 0 && f.blk0[1] == 128 && f.blk0[2] == 192 && f.blk0[3] == 224 && f.blk0[4] == 240);
    // grouped bins: regions of the need rounded up to 256: 9000 -> 9216, 3000 -> 3072; LDS 4 regions
    LAUNCH(l[11], NK_GROUP16, 0, 256, 256, 36864, 7, 0, 1007, 7, 0);
    CHECK(l[11].wave_bytes == 9216);
    LAUNCH(l[12], NK_GROUP, 0, 256, 256, 12288, 6, 0, 1006, 6, 0);
    CHECK(l[12].wave_bytes == 3072);
    LAUNCH(l[13], NK_DIRECT, 0, 256, 256, 20480, 1, 0, 1001, 1, 0);
    for (int i = 0; i < 14; ++i) CHECK((l[i].wave_bytes != 0) == (i == 11 || i == 12) && (l[i].gbytes != 0) == (i == 0));
    check_rows(p, h);
    // 11 bins outside the fused tiny classes + their one launch + 2 splittable block bins
    CHECK(numeric_launches(h) == 14);

    // The split not taken (one stream, or too few products): each block bin whole, from its bin list,
    // sized by its largest row.  numeric_launches counts splittable bins, not splits taken: still 14.
    const NumPlan q = plan_numeric(h, shape(100000, false, false));
    CHECK(q.n == 12);
    LAUNCH(q.launch[0], NK_GLOBAL, 0, 128, 1024, 13504, 5, 0, 1005, 5, 0);
    LAUNCH(q.launch[1], NK_BLOCK1024, 0, 256, 1024, 135168, 4, 0, 1004, 4, 0);
    LAUNCH(q.launch[2], NK_BLOCK256, 0, 1008, 256, 47104, 3, 0, 1003, 3, 0);
    for (int i = 3; i < 12; ++i) CHECK(memcmp(&q.launch[i], &p.launch[i + 2], sizeof(NumLaunch)) == 0);
    check_rows(q, h);
    CHECK(numeric_launches(h) == 14);
}

static void test_fused_copy() {
    // slot rows (tiny classes 0..3: 5000, 3000, 100, 10 rows) and 2000 small hash rows, nothing else
    Stats h{};
    h.num_count[8] = 5000;
    h.num_count[9] = 3000;
    h.num_count[10] = 100;
    h.num_count[11] = 10;
    h.num_count[14] = 2000;
    NumPlan p = plan_numeric(h, shape(100000, true, false));
    CHECK(p.n == 1);
    // the median of the 8110 slot rows is in class 0: 4 lanes, 64 rows a block over all of A's rows:
    // ceil(100000 / 64) = 1563 -> 1568 blocks; hash: ceil(2000 / 4) = 500 -> 504 blocks in front
    LAUNCH(p.launch[0], NK_COPY_HASH, 4, 2072, 256, 20480, 14, 0, 2000, 14, 0);
    CHECK(p.launch[0].hash_blocks == 504);
    const TinyFused& f = p.launch[0].fused;
    CHECK(f.nclass == 4 && f.c[0] == 3 && f.c[3] == 0 && f.count[0] == 10 && f.count[1] == 100 &&
          f.count[2] == 3000 && f.count[3] == 5000 && f.blk0[4] == 0);
    check_rows(p, h);
    CHECK(numeric_launches(h) == 2);  // (the fusion is not in its rule)
    // one row in the 10 KiB direct bin: the copy, the hash bin and that bin, each on its own
    h.num_count[2] = 1;
    p = plan_numeric(h, shape(100000, true, false));
    CHECK(p.n == 3);
    LAUNCH(p.launch[0], NK_COPY, 4, 1568, 256, 0, LIST_CLASSES, 0, 8110, 0, 0);
    LAUNCH(p.launch[1], NK_HASH, 0, 504, 256, 20480, 14, 0, 2000, 14, 0);
    LAUNCH(p.launch[2], NK_DIRECT16, 0, 8, 256, 40960, 2, 0, 1, 2, 0);
    check_rows(p, h);
    // lanes: the median row's class, at most 16.  1 + 9 rows: the median is in class 3 (32 lanes).
    // 16 rows a block: ceil(100000 / 16) = 6250 -> 6256
    Stats g{};
    g.num_count[8] = 1;
    g.num_count[11] = 9;
    p = plan_numeric(g, shape(100000, true, false));
    CHECK(p.n == 1);
    LAUNCH(p.launch[0], NK_COPY, 16, 6256, 256, 0, LIST_CLASSES, 0, 10, 0, 0);
    // ... the copy's block cap: 16384 below 2^22 rows, 65536 from there (2^22 / 16 = 262144 blocks)
    p = plan_numeric(g, shape((1 << 22) - 1, true, false));
    CHECK(p.launch[0].grid == 16384);
    p = plan_numeric(g, shape(1 << 22, true, false));
    CHECK(p.launch[0].grid == 65536);
    // without slot rows the same Stats compute classes 3 and 0: ceil(9 / 8) -> 8 blocks, ceil(1 / 64) -> 8
    p = plan_numeric(g, shape(100000, false, false));
    CHECK(p.n == 1);
    LAUNCH(p.launch[0], NK_TINY_SMALL, 0, 16, 256, 8192, LIST_CLASSES, 0, 10, 0, 0);
    CHECK(p.launch[0].fused.nclass == 2 && p.launch[0].fused.blk0[1] == 8 && p.launch[0].fused.blk0[2] == 16);
    // slot rows on, but classes 0..3 empty: no copy and no fused tiny launch
    Stats e{};
    e.num_count[14] = 2000;
    e.num_count[1] = 4;
    p = plan_numeric(e, shape(100000, true, false));
    CHECK(p.n == 2);
    LAUNCH(p.launch[0], NK_HASH, 0, 504, 256, 20480, 14, 0, 2000, 14, 0);
    LAUNCH(p.launch[1], NK_DIRECT, 0, 8, 256, 20480, 1, 0, 4, 1, 0);
}

static void test_sparse_and_edges() {
    Stats h{};
    h.num_count[1] = 5;
    NumPlan p = plan_numeric(h, shape(7, false, true));
    CHECK(p.n == 1);
    LAUNCH(p.launch[0], NK_DIRECT, 0, 8, 256, 20480, 1, 0, 5, 1, 0);
    // nothing to launch: counts of zero, or negative
    Stats z{};
    CHECK(plan_numeric(z, shape(0, false, true)).n == 0 && numeric_launches(z) == 0);
    for (int b = 0; b < 16; ++b) z.num_count[b] = -1;
    CHECK(plan_numeric(z, shape(100, true, true)).n == 0 && numeric_launches(z) == 0);
    // a block bin whose need was not recorded takes its budget: 64 KiB, and 160 KiB - 1024
    Stats k{};
    k.num_count[3] = 10;
    k.num_count[4] = 10;
    p = plan_numeric(k, shape(100, false, true));
    CHECK(p.n == 2);
    LAUNCH(p.launch[0], NK_BLOCK1024, 0, 16, 1024, 162816, 4, 0, 10, 4, 0);
    LAUNCH(p.launch[1], NK_BLOCK256, 0, 16, 256, 65536, 3, 0, 10, 3, 0);
    // ... and a need past the budget stops there
    k.num_block_need[0] = 70000;
    k.num_block_need[1] = 160000;
    p = plan_numeric(k, shape(100, false, true));
    CHECK(p.launch[0].lds == 162816 && p.launch[1].lds == 65536);
    // the small hash bin's block cap: 16384 below 2^21 rows, 65536 from there (2^21 / 4 = 524288 blocks)
    Stats w{};
    w.num_count[14] = (1 << 21) - 1;
    CHECK(plan_numeric(w, shape(1 << 22, false, false)).launch[0].grid == 16384);
    w.num_count[14] = 1 << 21;
    CHECK(plan_numeric(w, shape(1 << 22, false, false)).launch[0].grid == 65536);
    // the 10 KiB hash bin takes every row from the cursor up to 32768 rows (8192 blocks: capped at 2048)
    Stats q{};
    q.num_count[15] = 32768;
    p = plan_numeric(q, shape(1 << 20, false, false));
    CHECK(p.n == 1 && p.launch[0].qall == 1 && p.launch[0].grid == 2048);
    q.num_count[15] = 32769;
    CHECK(plan_numeric(q, shape(1 << 20, false, false)).launch[0].qall == 0);
    // 32-bit gather offsets while nnz(B) (+ 3 nnz(A) with B's union rows) < 2^29
    NumShape sh = shape(100, false, false);
    sh.nnzA = 100;
    sh.nnzB = (1 << 29) - 1;
    CHECK(plan_numeric(h, sh).o32 == 1);
    sh.nnzB = 1 << 29;
    CHECK(plan_numeric(h, sh).o32 == 0);
    sh.nnzB = (1 << 29) - 300;
    CHECK(plan_numeric(h, sh).o32 == 1);
    sh.bx_on = 1;  // 2^29 - 300 + 300
    CHECK(plan_numeric(h, sh).o32 == 0);
    sh.nnzB = (1 << 29) - 301;
    CHECK(plan_numeric(h, sh).o32 == 1);
}

// Speculation's premise: the plan is a function of what stats_same_plan compares.  plan_numeric
// reads num_count, num_global_need, num_block_need, num_block_small_need, num_block_big and
// num_wave_need -- each of them compared there; the fields it does not compare change nothing.
static void test_speculation_premise() {
    const Stats h = every_bin();
    const NumShape sh = shape(100000, false, true);
    const NumPlan p = plan_numeric(h, sh);
    Stats a = h;
    a.err = 8;
    CHECK(stats_same_plan(a, h) && same(plan_numeric(a, sh), p));
    a = h;
    a.scan_ticket = 77;
    CHECK(stats_same_plan(a, h) && same(plan_numeric(a, sh), p));
    a = h;
    a.final_done = 5;
    CHECK(stats_same_plan(a, h) && same(plan_numeric(a, sh), p));
    a = h;
    a.an_slots = 1ull << 40;
    CHECK(stats_same_plan(a, h) && same(plan_numeric(a, sh), p));
    a = h;
    a.an_other = 123456;
    CHECK(stats_same_plan(a, h) && same(plan_numeric(a, sh), p));
    a = h;
    a.an_done = 3;
    CHECK(stats_same_plan(a, h) && same(plan_numeric(a, sh), p));
    a.err = 1;  // all of them at once
    a.scan_ticket = 9;
    a.final_done = 2;
    a.an_slots = 4;
    a.an_other = 6;
    CHECK(stats_same_plan(a, h) && same(plan_numeric(a, sh), p));
    // and a change the plan depends on is one the comparison sees
    a = h;
    a.num_wave_need[0] = 3100;
    CHECK(!stats_same_plan(a, h) && !same(plan_numeric(a, sh), p));
    a = h;
    a.num_count[15] += 8;
    CHECK(!stats_same_plan(a, h) && !same(plan_numeric(a, sh), p));
}

static void test_dealing() {
    const int want3[14] = {0, 1, 2, 0, 1, 2, 0, 1, 2, 0, 1, 2, 0, 1};
    const int want4[14] = {0, 1, 2, 3, 0, 1, 2, 3, 0, 1, 2, 3, 0, 1};
    int a = 0, b = 0;  // launches of phase A (the call's stream) and phase B, as bits
    for (int i = 0; i < 14; ++i) {
        CHECK(stream_of(i, 1) == 0 && stream_of(i, 0) == 0);
        CHECK(stream_of(i, 3) == want3[i]);
        CHECK(stream_of(i, 4) == want4[i]);
        (stream_of(i, 4) == 0 ? a : b) |= 1 << i;
    }
    CHECK(a == 0x1111 && b == 0x2eee && (a & b) == 0 && (a | b) == 0x3fff);
}

// every field of a launch, one by one
static bool same_launch(const NumLaunch& a, const NumLaunch& b) {
    bool ok = a.kernel == b.kernel && a.variant == b.variant && a.grid == b.grid && a.block == b.block &&
              a.lds == b.lds && a.list_bin == b.list_bin && a.list_off == b.list_off && a.count == b.count &&
              a.slot == b.slot && a.wave_bytes == b.wave_bytes && a.gbytes == b.gbytes && a.qall == b.qall &&
              a.hash_blocks == b.hash_blocks && a.after_split == b.after_split && a.cursor_walk == b.cursor_walk &&
              a.fused.nclass == b.fused.nclass;
    for (int k = 0; k < 4; ++k) ok = ok && a.fused.c[k] == b.fused.c[k] && a.fused.count[k] == b.fused.count[k];
    for (int k = 0; k < 5; ++k) ok = ok && a.fused.blk0[k] == b.fused.blk0[k];
    return ok;
}

// NumShape::no_o32 (MHS_NO_O32=1): o32 == 0 below the size rule, and nothing else of the plan moves.
static void test_no_o32() {
    static_assert(sizeof(NumLaunch) == (15 + 14) * sizeof(int), "same_launch names every field of NumLaunch");
    struct Case {
        Stats h;
        NumShape sh;
    };
    Stats copy{};  // the fused copy (test_fused_copy)
    copy.num_count[8] = 5000;
    copy.num_count[9] = 3000;
    copy.num_count[14] = 2000;
    Stats cls3{};  // the plain copy, 16 lanes
    cls3.num_count[8] = 1;
    cls3.num_count[11] = 9;
    NumShape walk = shape(100000, false, false);  // the grouped cursor walk
    walk.cus = 256;
    walk.group_cap = 8;
    const Case cases[] = {{every_bin(), shape(100000, false, true)}, {every_bin(), shape(100000, false, false)},
                          {every_bin(), walk}, {copy, shape(100000, true, false)}, {cls3, shape(100000, true, false)},
                          {Stats{}, shape(0, false, false)}};
    for (const Case& c : cases) {
        NumShape on = c.sh;
        CHECK(on.no_o32 == 0);  // (the default: the size rule)
        const NumPlan p = plan_numeric(c.h, on);
        on.no_o32 = 1;
        const NumPlan q = plan_numeric(c.h, on);
        CHECK(p.o32 == 1 && q.o32 == 0 && p.n == q.n);
        for (int i = 0; i < NUM_PLAN_MAX; ++i) CHECK(same_launch(p.launch[i], q.launch[i]));
        NumPlan r = q;  // ... and bytewise, o32 apart
        r.o32 = 1;
        CHECK(same(p, r));
    }
    // above the size rule the switch changes nothing: o32 is 0 either way
    NumShape big = shape(100, false, false);
    big.nnzB = 1 << 29;
    const NumPlan p = plan_numeric(every_bin(), big);
    big.no_o32 = 1;
    CHECK(p.o32 == 0 && same(p, plan_numeric(every_bin(), big)));
}

int main() {
    test_no_o32();
    test_every_bin();
    test_fused_copy();
    test_sparse_and_edges();
    test_speculation_premise();
    test_dealing();
    if (failures) return 1;
    puts("numplan ok");
    return 0;
}
