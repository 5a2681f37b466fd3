// Host check of the pre-numeric launch plans (mh-spgemm_amd/csrc/mhs_frontplan.hpp): which kernels go
// out before the numeric phase, with which variants, grids, LDS and streams, and what a speculated plan
// leaves out.  A stand-alone program, built with -fsanitize=address,undefined by tests/test_host.py.
// Every expected figure below is a literal worked out by hand from the rules (the arithmetic is in
// the comments), none comes from the helpers under test.
#include "../mh-spgemm_amd/csrc/mhs_frontplan.hpp"

#include <cstdio>
#include <cstring>
#include <set>
#include <utility>

using namespace mhs;

static int failures = 0;
#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            ++failures;                                                 \
            fprintf(stderr, "line %d: %s\n", __LINE__, #cond);          \
        }                                                               \
    } while (0)

static_assert(sizeof(FrontLaunch) == 16 * sizeof(int), "ints only, no padding: plans compare bytewise");
static bool same(const FrontPlan& a, const FrontPlan& b) { return memcmp(&a, &b, sizeof(FrontPlan)) == 0; }

// one expected launch: the fields every kind has (the rest are checked where they matter)
struct Want {
    int kernel, variant, grid, block, lds, stream;
};
static void check_launch(const FrontLaunch& l, const Want& w, int line) {
    const bool ok = l.kernel == w.kernel && l.variant == w.variant && l.grid == w.grid &&
                    l.block == w.block && l.lds == w.lds && l.stream == w.stream;
    if (!ok) {
        ++failures;
        fprintf(stderr, "line %d: launch {k %d v %d grid %d block %d lds %d stream %d}\n", line, l.kernel,
                l.variant, l.grid, l.block, l.lds, l.stream);
    }
}
#define LAUNCH(l, ...) check_launch(l, Want{__VA_ARGS__}, __LINE__)

// FrontShape: M, MB, nnzA, nnzB, mask, probe, nft, sym_big, near, fork
static FrontShape rows_shape(int avgA, int avgB) { return FrontShape{1000, 1000, avgA, avgB, 1, 0, 0, 0, 0, 0}; }

// ---- k_mask_b / k_mask_lane and k_analyze / k_analyze_lane on both sides of every edge: 1000 rows,
// nnz = 1000 avg + 999 (the largest count of that floor average) or 1000 avg (the smallest)
static void geometry_edges() {
    struct Edge {
        int nnz;
        Want mask, analyze;
        int words;
    };
    // lane kernels: 256 rows a block, ceil(1000 / 256) = 4 blocks, two per-block words each = 8.
    // groups of G lanes: 256 / G rows a block -- G = 8: ceil(1000 / 32) = 32; 16: ceil(1000 / 16) = 63;
    // 32: ceil(1000 / 8) = 125; 64: 1000 / 4 = 250.  k_analyze stays at 8 lanes (MHS_AN_GMAX): 32 blocks, 32 words.
    const Edge edges[] = {
        // average 3 | 4: the lane kernels load 4 | 8 entries at a time
        {3999, {FK_MASK_LANE, 4, 4, 256, 0, 0}, {FK_ANALYZE_LANE, 4, 4, 256, 0, 0}, 8},
        {4000, {FK_MASK_LANE, 8, 4, 256, 0, 0}, {FK_ANALYZE_LANE, 8, 4, 256, 0, 0}, 8},
        // average 8 | 9: MHS_LANE_AVG, a lane per row | 8 lanes per row, four chunks a round trip
        {8999, {FK_MASK_LANE, 8, 4, 256, 0, 0}, {FK_ANALYZE_LANE, 8, 4, 256, 0, 0}, 8},
        {9000, {FK_MASK, 8, 32, 256, 0, 0}, {FK_ANALYZE, 8, 32, 256, 0, 0}, 32},
        // the mask's groups widen to 2 G once 2 G <= avg / 8: 127 / 8 = 15 < 16 | 128 / 8 = 16
        {127999, {FK_MASK, 8, 32, 256, 0, 0}, {FK_ANALYZE, 8, 32, 256, 0, 0}, 32},
        {128000, {FK_MASK, 16, 63, 256, 0, 0}, {FK_ANALYZE, 8, 32, 256, 0, 0}, 32},
        // 255 / 8 = 31 < 32 | 256 / 8 = 32
        {255999, {FK_MASK, 16, 63, 256, 0, 0}, {FK_ANALYZE, 8, 32, 256, 0, 0}, 32},
        {256000, {FK_MASK, 32, 125, 256, 0, 0}, {FK_ANALYZE, 8, 32, 256, 0, 0}, 32},
        // 511 / 8 = 63 < 64 | 512 / 8 = 64: the whole wave
        {511999, {FK_MASK, 32, 125, 256, 0, 0}, {FK_ANALYZE, 8, 32, 256, 0, 0}, 32},
        {512000, {FK_MASK, 64, 250, 256, 0, 0}, {FK_ANALYZE, 8, 32, 256, 0, 0}, 32},
    };
    for (const Edge& e : edges) {
        const FrontPlan p = plan_front_rows(rows_shape(e.nnz, e.nnz));
        CHECK(p.n == 3 && p.fork == 0 && p.left_out == 0);
        check_launch(p.launch[0], e.mask, __LINE__);
        check_launch(p.launch[1], e.analyze, __LINE__);
        CHECK(p.launch[1].words == e.words && analyze_launch(e.nnz, 1000).words == e.words);
        LAUNCH(p.launch[2], FK_BIN_LIST, 1, 1, 1024, 0, 0);  // ceil(1000 / 1024) = 1 block of 1024 rows
    }
    // the lane kernels' doubled words where the blocks are not a round number: 257 rows of one entry,
    // ceil(257 / 256) = 2 blocks, 4 words; the workspace reserves them for no rows at all too (0)
    CHECK(analyze_launch(257, 257).grid == 2 && analyze_launch(257, 257).words == 4);
    CHECK(analyze_launch(0, 0).grid == 0 && analyze_launch(0, 0).words == 0);
    // 8 lanes: ceil(257 / 32) = 9 blocks, one word each
    CHECK(analyze_launch(257 * 70, 257).grid == 9 && analyze_launch(257 * 70, 257).words == 9);
}

// ---- the stages of the first plan: no mask on a later chunk, none for an empty B; the probe's
// publication between k_analyze and k_bin_list, summing k_analyze's words; no rows: the mask alone
static void rows_stages() {
    FrontShape sh = rows_shape(9000, 9000);
    sh.mask = 0;
    FrontPlan p = plan_front_rows(sh);
    CHECK(p.n == 2 && p.launch[0].kernel == FK_ANALYZE && p.launch[1].kernel == FK_BIN_LIST);
    sh.mask = 1;
    sh.MB = 0;
    CHECK(plan_front_rows(sh).n == 2 && plan_front_rows(sh).launch[0].kernel == FK_ANALYZE);
    sh = rows_shape(3999, 9000);
    sh.probe = 1;
    p = plan_front_rows(sh);
    CHECK(p.n == 4);
    LAUNCH(p.launch[1], FK_ANALYZE_LANE, 4, 4, 256, 0, 0);
    LAUNCH(p.launch[2], FK_PROBE_PUBLISH, 0, 64, 1024, 0, 0);
    CHECK(p.launch[2].words == 8);  // (the lane kernel's 2 x 4)
    LAUNCH(p.launch[3], FK_BIN_LIST, 1, 1, 1024, 0, 0);
    sh = rows_shape(0, 9000);
    sh.M = 0;
    p = plan_front_rows(sh);
    CHECK(p.n == 1 && p.launch[0].kernel == FK_MASK);
    CHECK(plan_front_symbolic(sh, nullptr).n == 0);
}

// ---- k_bin_list / k_scan: 1024 rows a block below 2^19 rows, 4096 from there
static void scan_width() {
    // M = 2^19 - 1 = 524287: k_scan walks M + 1 = 524288 words = 512 blocks of 1024; k_bin_list ceil(524287 / 1024) = 512
    LAUNCH(front_scan(524287), FK_SCAN, 1, 512, 1024, 0, 0);
    FrontShape sh{524287, 0, 524287, 0, 0, 0, 0, 0, 0, 0};
    LAUNCH(plan_front_rows(sh).launch[1], FK_BIN_LIST, 1, 512, 1024, 0, 0);
    // M = 2^19: k_scan ceil(524289 / 4096) = 129; k_bin_list 524288 / 4096 = 128
    LAUNCH(front_scan(524288), FK_SCAN, 4, 129, 1024, 0, 0);
    sh.M = sh.nnzA = 524288;
    LAUNCH(plan_front_rows(sh).launch[1], FK_BIN_LIST, 4, 128, 1024, 0, 0);
    LAUNCH(front_scan(1), FK_SCAN, 1, 1, 1024, 0, 0);
}

static bool zero_roles(const FrontLaunch& l) {
    for (int c = 0; c <= 5; ++c)
        if (l.blk0[c] != 0) return false;
    return true;
}

// Symbolic bins: WAVE 1, B256 2, B1024 3, GLOBAL 4, tiny classes 0..5 at 5..10, WM 11.
// ---- k_sym_common, LDS 4 waves x 5120 = 20480
static void sym_common() {
    // no plan, 1000 rows: every role sized for M -- wave rows ceil(1000 / 4) = 250 -> 256 blocks (multiple of 8),
    // tiny classes 5 x 1024 = 5120 blocks at fixed places (no role table)
    FrontShape sh{1000, 1000, 9000, 9000, 1, 0, 0, 0, 0, 0};
    FrontPlan p = plan_front_symbolic(sh, nullptr);
    CHECK(p.n == 3 && p.left_out == 0 && p.fork == 0);
    LAUNCH(p.launch[0], FK_SYM_COMMON, 0, 5376, 256, 20480, 0);
    CHECK(p.launch[0].wave_blocks == 256 && zero_roles(p.launch[0]));
    LAUNCH(p.launch[1], FK_SYM_RARE, 0, 256, 1024, 162816, 0);  // 160 KiB - 1024
    LAUNCH(p.launch[2], FK_SYM_B256, 0, 1000, 256, 32768, 0);   // M blocks (cap 1024), a multiple of 8
    sh.M = 3000;  // past the 256-thread bin's cap
    LAUNCH(plan_front_symbolic(sh, nullptr).launch[2], FK_SYM_B256, 0, 1024, 256, 32768, 0);

    // a plan (no slots): WAVE = 1000 rows -> 256 blocks; tiny classes all or none
    Stats h{};
    h.sym_count[1] = 1000;
    h.sym_count[7] = 3;  // class 2
    h.sym_count[11] = 1;  // (the rare launch stays: see skip_rules)
    h.sym_count[2] = 1;
    sh.M = 1000;
    p = plan_front_symbolic(sh, &h);
    LAUNCH(p.launch[0], FK_SYM_COMMON, 0, 5376, 256, 20480, 0);
    CHECK(p.launch[0].wave_blocks == 256 && zero_roles(p.launch[0]));
    h.sym_count[1] = 0;  // an empty wave bin: no wave blocks
    p = plan_front_symbolic(sh, &h);
    LAUNCH(p.launch[0], FK_SYM_COMMON, 0, 5120, 256, 20480, 0);
    CHECK(p.launch[0].wave_blocks == 0);
    h.sym_count[1] = 1000;
    h.sym_count[7] = 0;  // every tiny class empty: no tiny blocks
    p = plan_front_symbolic(sh, &h);
    LAUNCH(p.launch[0], FK_SYM_COMMON, 0, 256, 256, 20480, 0);
    CHECK(p.launch[0].wave_blocks == 256);
    h.sym_count[9] = 2;  // class 4 (the scattered rows) counts as a tiny class
    CHECK(plan_front_symbolic(sh, &h).launch[0].grid == 5376);
    h.sym_count[9] = 0;
    h.sym_count[1] = 0;  // both empty: no k_sym_common at all
    p = plan_front_symbolic(sh, &h);
    CHECK(p.n == 2 && p.launch[0].kernel == FK_SYM_RARE && p.launch[1].kernel == FK_SYM_B256 && p.left_out == 0);

    // numeric-first slots, no plan: class c (4, 8, 16, 32 lanes a row: 64, 32, 16, 8 rows a block) sized for M
    // rows, capped at 4096 blocks below 2^22 rows and 16384 from there; class 4 a fixed 1024.
    // M = 2^22 - 1: the smallest class needs ceil(4194303 / 64) = 65536 > 4096 blocks, so all four are capped.
    FrontShape big{4194303, 1000, 9000000, 9000, 1, 1, 1, 0, 0, 0};
    p = plan_front_symbolic(big, nullptr);
    const int below[6] = {0, 4096, 8192, 12288, 16384, 17408};
    CHECK(memcmp(p.launch[0].blk0, below, sizeof below) == 0);
    // wave rows: ceil(M / 4) > 2048 -> 2048; grid 2048 + 17408
    LAUNCH(p.launch[0], FK_SYM_COMMON, 0, 19456, 256, 20480, 0);
    CHECK(p.launch[0].wave_blocks == 2048);
    big.M = 4194304;  // 65536 > 16384: capped again
    p = plan_front_symbolic(big, nullptr);
    const int from[6] = {0, 16384, 32768, 49152, 65536, 66560};
    CHECK(memcmp(p.launch[0].blk0, from, sizeof from) == 0);
    LAUNCH(p.launch[0], FK_SYM_COMMON, 0, 68608, 256, 20480, 0);  // 2048 + 66560
    big.sym_big = 1;  // the probe counted 2^21 table rows: wave cap 65536 < ceil(M / 4) = 1048576
    p = plan_front_symbolic(big, nullptr);
    LAUNCH(p.launch[0], FK_SYM_COMMON, 0, 132096, 256, 20480, 0);  // 65536 + 66560
    CHECK(p.launch[0].wave_blocks == 65536);

    // slots with a plan (an unprobed numeric-first call), class 1 empty:
    // WAVE 1000 -> 256; class 0: 6400 rows / 64 = 100 -> 104; class 1: 0; class 2: 100 rows / 16 = 7 -> 8;
    // class 3: 9 rows / 8 = 2 -> 8; class 4 empty: no walk
    FrontShape nf{100000, 1000, 300000, 9000, 1, 0, 1, 0, 0, 0};
    Stats s{};
    s.sym_count[1] = 1000;
    s.sym_count[5] = 6400;
    s.sym_count[7] = 100;
    s.sym_count[8] = 9;
    p = plan_front_symbolic(nf, &s);
    const int roles[6] = {0, 104, 104, 112, 120, 120};
    CHECK(memcmp(p.launch[0].blk0, roles, sizeof roles) == 0);
    LAUNCH(p.launch[0], FK_SYM_COMMON, 0, 376, 256, 20480, 0);  // 256 + 120
    s.sym_count[9] = 5;  // class 4: its 1024 blocks
    p = plan_front_symbolic(nf, &s);
    CHECK(p.launch[0].blk0[4] == 120 && p.launch[0].blk0[5] == 1144 && p.launch[0].grid == 1400);
}

// ---- what an unforked speculated plan leaves out
static void skip_rules() {
    FrontShape sh{1000, 1000, 9000, 9000, 1, 0, 0, 0, 0, 0};
    Stats h{};
    h.sym_count[1] = 1000;
    // every rare bin and the 256-thread bin empty: k_sym_common alone, two launches left out
    FrontPlan p = plan_front_symbolic(sh, &h);
    CHECK(p.n == 1 && p.launch[0].kernel == FK_SYM_COMMON && p.left_out == 2);
    for (int bin : {11, 3, 4}) {  // WM, B1024, GLOBAL: each keeps the rare launch
        Stats k = h;
        k.sym_count[bin] = 1;
        p = plan_front_symbolic(sh, &k);
        CHECK(p.n == 2 && p.left_out == 1);
        LAUNCH(p.launch[1], FK_SYM_RARE, 0, 256, 1024, 162816, 0);
        CHECK(p.launch[1].with_near == 0);
    }
    // near candidates keep it where near groups are planned (it runs the near check), not elsewhere
    Stats k = h;
    k.near_heads = 7;
    p = plan_front_symbolic(sh, &k);
    CHECK(p.n == 1 && p.left_out == 2);
    sh.near = 1;
    p = plan_front_symbolic(sh, &k);
    CHECK(p.n == 2 && p.left_out == 1 && p.launch[1].kernel == FK_SYM_RARE && p.launch[1].with_near == 1);
    p = plan_front_symbolic(sh, &h);  // planned, no candidates
    CHECK(p.n == 1 && p.left_out == 2);
    // the 256-thread bin on its own count
    k = h;
    k.sym_count[2] = 1;
    p = plan_front_symbolic(sh, &k);
    CHECK(p.n == 2 && p.left_out == 1);
    LAUNCH(p.launch[1], FK_SYM_B256, 0, 1000, 256, 32768, 0);
    k.sym_count[3] = 4;
    p = plan_front_symbolic(sh, &k);
    CHECK(p.n == 3 && p.left_out == 0 && p.launch[1].kernel == FK_SYM_RARE && p.launch[2].kernel == FK_SYM_B256);
    // no plan: nothing left out, the near check inside k_sym_rare
    p = plan_front_symbolic(sh, nullptr);
    CHECK(p.n == 3 && p.left_out == 0 && p.launch[1].with_near == 1);
    sh.M = 1;  // (a group needs two rows)
    CHECK(plan_front_symbolic(sh, nullptr).launch[1].with_near == 0);
}

// ---- a forked pass: k_sym_common on the call's stream, the rare bins on the aux stream, the 256-thread
// bin on the call's stream, the join, k_near; nothing left out, whatever the plan's bins hold
static void forked() {
    FrontShape sh{1000, 1000, 9000, 9000, 1, 0, 0, 0, 1, 1};
    Stats h{};
    h.sym_count[1] = 1000;
    for (const Stats* spec : {(const Stats*)nullptr, (const Stats*)&h}) {
        const FrontPlan p = plan_front_symbolic(sh, spec);
        CHECK(p.n == 4 && p.fork == 1 && p.left_out == 0);
        // (a plan with the tiny classes empty: 256 wave blocks alone)
        LAUNCH(p.launch[0], FK_SYM_COMMON, 0, spec ? 256 : 5376, 256, 20480, FRONT_CALL);
        LAUNCH(p.launch[1], FK_SYM_RARE, 0, 256, 1024, 162816, FRONT_AUX);
        LAUNCH(p.launch[2], FK_SYM_B256, 0, 1000, 256, 32768, FRONT_CALL);
        // k_near: a wave per three rows -- 333 waves = ceil(333 / 4) = 84 -> 88 blocks (cap 2048)
        LAUNCH(p.launch[3], FK_NEAR, 0, 88, 256, 0, FRONT_CALL);
        CHECK(p.launch[1].with_near == 0);
        CHECK(!p.launch[0].after_join && !p.launch[1].after_join && !p.launch[2].after_join && p.launch[3].after_join);
    }
    sh.M = 100000;  // 33333 waves = 8334 blocks > 2048
    CHECK(plan_front_symbolic(sh, nullptr).launch[3].grid == 2048);
    sh.near = 0;  // no near groups: no k_near, the join behind the last launch
    const FrontPlan p = plan_front_symbolic(sh, nullptr);
    CHECK(p.n == 3 && p.fork == 1 && p.launch[1].stream == FRONT_AUX && !p.launch[2].after_join);
    sh.M = 0;  // no rows: the fork and join alone
    CHECK(plan_front_symbolic(sh, nullptr).n == 0 && plan_front_symbolic(sh, nullptr).fork == 1);
}

// ---- a row chunk's pass is the unforked plan without a speculated plan or near groups
static void chunked() {
    const FrontShape chunk{1000, 1000, 9000, 9000, 1};  // (as front_pass spells it)
    const FrontShape whole{1000, 1000, 9000, 9000, 1, 0, 0, 0, 0, 0};
    CHECK(same(plan_front_rows(chunk), plan_front_rows(whole)));
    const FrontPlan p = plan_front_symbolic(chunk, nullptr);
    CHECK(same(p, plan_front_symbolic(whole, nullptr)));
    CHECK(p.n == 3 && p.fork == 0 && p.left_out == 0 && p.launch[0].kernel == FK_SYM_COMMON &&
          p.launch[1].kernel == FK_SYM_RARE && p.launch[1].with_near == 0 && p.launch[1].stream == FRONT_CALL &&
          p.launch[2].kernel == FK_SYM_B256);
    // near groups change that launch's with_near and nothing else
    FrontShape near = whole;
    near.near = 1;
    FrontPlan q = plan_front_symbolic(near, nullptr);
    CHECK(!same(p, q));
    q.launch[1].with_near = 0;
    CHECK(same(p, q));
}

// ---- every average row length that can change the geometry (the widest group is reached at 512), both
// floor-equal extremes of nnz, rows on both sides of every M threshold: the variants reached are exactly
// those issue_front (mhs_kernels.hip) instantiates -- the list below is its switch arms
static void sweep() {
    std::set<std::pair<int, int>> reached;
    const int Ms[] = {1, 255, 256, 257, 1000, 524287, 524288, 4194303, 4194304};
    for (int M : Ms) {
        for (long long avg = 0; avg <= 4096; ++avg)
            for (long long nnz : {avg * M, avg * M + M - 1}) {
                const FrontLaunch m = mask_launch(nnz, M), a = analyze_launch(nnz, M);
                reached.insert({m.kernel, m.variant});
                reached.insert({a.kernel, a.variant});
                // a lane per row: 256 rows a block; groups of `variant` lanes: 256 / variant
                const int mrows = m.kernel == FK_MASK_LANE ? 256 : 256 / m.variant;
                const int arows = a.kernel == FK_ANALYZE_LANE ? 256 : 256 / a.variant;
                CHECK(m.grid == (M + mrows - 1) / mrows && m.grid > 0 && m.block == 256 && m.lds == 0);
                CHECK(a.grid == (M + arows - 1) / arows && a.block == 256 && a.lds == 0 &&
                      a.words == (a.kernel == FK_ANALYZE_LANE ? 2 : 1) * a.grid);
            }
        reached.insert({FK_BIN_LIST, scan_per(M)});
        reached.insert({FK_SCAN, front_scan(M).variant});
    }
    const std::set<std::pair<int, int>> want = {
        {FK_MASK_LANE, 4}, {FK_MASK_LANE, 8}, {FK_MASK, 8}, {FK_MASK, 16}, {FK_MASK, 32}, {FK_MASK, 64},
        {FK_ANALYZE_LANE, 4}, {FK_ANALYZE_LANE, 8}, {FK_ANALYZE, 8},
        {FK_BIN_LIST, 1}, {FK_BIN_LIST, 4}, {FK_SCAN, 1}, {FK_SCAN, 4}};
    CHECK(reached == want);
}

static void determinism() {
    FrontShape sh{100000, 5000, 300000, 90000, 1, 0, 1, 0, 0, 0};
    Stats h{};
    h.sym_count[1] = 1000;
    h.sym_count[5] = 6400;
    h.sym_count[11] = 2;
    CHECK(same(plan_front_rows(sh), plan_front_rows(sh)));
    CHECK(same(plan_front_symbolic(sh, &h), plan_front_symbolic(sh, &h)));
    const FrontLaunch a = front_scan(100000), b = front_scan(100000);
    CHECK(memcmp(&a, &b, sizeof a) == 0);
    Stats k = h;  // fields the plans do not read leave them alone
    k.flop = 12345;
    k.num_count[3] = 9;
    CHECK(same(plan_front_symbolic(sh, &h), plan_front_symbolic(sh, &k)));
}

int main() {
    geometry_edges();
    rows_stages();
    scan_width();
    sym_common();
    skip_rules();
    forked();
    chunked();
    sweep();
    determinism();
    if (failures) {
        fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    puts("frontplan ok");
    return 0;
}
