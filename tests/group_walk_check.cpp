// Host check of the grouped numeric bin's cursor walk: the launch plan_numeric gives the NUM_WSG
// bin (mh-spgemm_amd/csrc/mhs_numplan.hpp) and the take rule its waves follow
// (mh-spgemm_amd/csrc/mhs_groupwalk.hpp).  A stand-alone program, built with
// -fsanitize=address,undefined by tests/test_group_walk_host.py.  Expected figures are literals
// worked out by hand (the arithmetic is in the comments).
#include "../mh-spgemm_amd/csrc/mhs_numplan.hpp"

#include <cstdio>
#include <vector>

using namespace mhs;

static int failures = 0;
#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            ++failures;                                                 \
            fprintf(stderr, "line %d: %s\n", __LINE__, #cond);          \
        }                                                               \
    } while (0)

static const NumLaunch* group_launch(const NumPlan& p) {
    for (int i = 0; i < p.n; ++i)
        if (p.launch[i].kernel == NK_GROUP) return &p.launch[i];
    return nullptr;
}

static NumPlan plan_wsg(int count, int need, int cus, int cap) {
    Stats h{};
    h.num_count[NUM_WSG] = count;
    h.num_wave_need[0] = need;
    NumShape sh{100000, 1000, 1000, 0, 0, 0, 128};
    sh.cus = cus;
    sh.group_cap = cap;
    return plan_numeric(h, sh);
}

static void test_plan() {
    // 256 CUs, regions of 3000 -> 3072 bytes: the LDS would hold 163840 / (4 * 3072) = 13 blocks a
    // CU, the 4 waves per SIMD hold 4: a resident set of 1024 blocks (4096 waves)
    CHECK(group_resident_blocks(256, 3072) == 1024);
    CHECK(group_resident_blocks(256, 10240) == 1024);  // 163840 / 40960 = 4
    CHECK(group_resident_blocks(256, 20480) == 512);   // (2 blocks a CU by LDS)
    CHECK(group_resident_blocks(304, 0) == 1216);
    // 1006 groups: ceil(1006 / 4) = 252 -> 256 blocks, fewer than the resident set: the static walk
    NumPlan p = plan_wsg(1006, 3000, 256, 0);
    const NumLaunch* l = group_launch(p);
    CHECK(p.n == 1 && l && l->grid == 256 && l->cursor_walk == 0 && l->count == 1006 && l->slot == NUM_WSG);
    CHECK(l && l->wave_bytes == 3072 && l->lds == 12288 && l->block == 256);
    // 20,817 groups: ceil / 4 = 5205 blocks > 1024: the resident set, groups from the cursors
    p = plan_wsg(20817, 3000, 256, 0);
    l = group_launch(p);
    CHECK(p.n == 1 && l && l->grid == 1024 && l->cursor_walk == 1 && l->count == 20817 && l->slot == NUM_WSG);
    CHECK(l && l->wave_bytes == 3072 && l->lds == 12288);
    // exactly the resident set (4096 groups, 1024 blocks): still a wave a group, static
    l = group_launch(p = plan_wsg(4096, 3000, 256, 0));
    CHECK(l && l->grid == 1024 && l->cursor_walk == 0);
    l = group_launch(p = plan_wsg(4097, 3000, 256, 0));  // 1025 blocks
    CHECK(l && l->grid == 1024 && l->cursor_walk == 1);
    // the compute units not known: today's grid, capped at 4096 blocks
    l = group_launch(p = plan_wsg(20817, 3000, 0, 0));
    CHECK(l && l->grid == 4096 && l->cursor_walk == 0);
    // a device of more CUs than the launch's block cap allows resident: 4096 stays the cap
    l = group_launch(p = plan_wsg(1 << 20, 3000, 2048, 0));
    CHECK(l && l->grid == 4096 && l->cursor_walk == 1);
    // the cap option: 8 blocks for 301 groups, and for 20 (5 blocks -> 8: 32 waves, 12 of them idle),
    // each from the cursors
    l = group_launch(p = plan_wsg(301, 3000, 256, 8));
    CHECK(l && l->grid == 8 && l->cursor_walk == 1 && l->count == 301);
    l = group_launch(p = plan_wsg(20, 3000, 256, 8));
    CHECK(l && l->grid == 8 && l->cursor_walk == 1);
    l = group_launch(p = plan_wsg(301, 3000, 0, 8));  // (the cap alone turns the walk on)
    CHECK(l && l->grid == 8 && l->cursor_walk == 1);
    l = group_launch(p = plan_wsg(301, 3000, 256, 12));  // caps round up to a multiple of 8
    CHECK(l && l->grid == 16 && l->cursor_walk == 1);
    // the plan stays a function of what stats_same_plan compares
    Stats a{}, b{};
    a.num_count[NUM_WSG] = 20817;
    b.num_count[NUM_WSG] = 20818;
    CHECK(!stats_same_plan(a, b));
}

// The rule alone: the eighths tile [0, count); an eighth's static rounds and its tickets tile the
// eighth; tickets map into [split, end) in order, and everything from there on is "none".
static void test_rule(int count, int blocks) {
    int covered = 0;
    for (int g = 0; g < 8; ++g) {
        const GroupWalk w = group_walk(count, g, blocks);
        CHECK(w.begin == covered && w.begin <= w.split && w.split <= w.end && w.waves == blocks / 8 * 4);
        CHECK(w.begin == group_begin(count, g) && w.end == group_begin(count, g + 1));
        covered = w.end;
        // whole rounds only, and between one and two rounds (or the whole short eighth) left to the cursor
        CHECK((w.split - w.begin) % w.waves == 0);
        CHECK(w.end - w.split < 2 * w.waves && (w.split == w.begin || w.end - w.split >= w.waves));
        for (int t = 0; t < w.end - w.split; ++t) CHECK(group_take(w, t) == w.split + t);
        CHECK(group_take(w, w.end - w.split) == GROUP_NONE);
        CHECK(group_take(w, w.end - w.split + 1) == GROUP_NONE);
        CHECK(group_take(w, w.end - w.split + 70000) == GROUP_NONE);
        CHECK(group_take(w, 0x7fffffff) == GROUP_NONE);
    }
    CHECK(covered == count);
}
// hand-worked: 20,817 groups on 1,024 blocks: eighth 0 is [0, 2602), 512 waves, 5 full rounds:
// 4 static (2048 indices), 554 tickets; on 8 blocks (4 waves): 650 rounds, 649 static
static void test_rule_literals() {
    GroupWalk w = group_walk(20817, 0, 1024);
    CHECK(w.begin == 0 && w.end == 2602 && w.waves == 512 && w.split == 2048);
    CHECK(group_static_first(w, 0) == 0 && group_static_first(w, 511) == 511);
    CHECK(group_static_next(w, 511) == 1023 && group_static_next(w, 1535) == 2047 && group_static_next(w, 1536) == GROUP_NONE);
    CHECK(group_take(w, 0) == 2048 && group_take(w, 553) == 2601 && group_take(w, 554) == GROUP_NONE);
    w = group_walk(20817, 7, 1024);  // [18214, 20817): 2603 entries
    CHECK(w.begin == 18214 && w.end == 20817 && w.split == 18214 + 2048 && group_take(w, 554) == 20816);
    w = group_walk(20817, 0, 8);
    CHECK(w.waves == 4 && w.split == 2596 && group_take(w, 5) == 2601 && group_take(w, 6) == GROUP_NONE);
    w = group_walk(7, 3, 8);  // [2, 3): one entry, four waves: no static round
    CHECK(w.begin == 2 && w.end == 3 && w.split == 2 && group_static_first(w, 0) == GROUP_NONE && group_take(w, 0) == 2);
}

// The walk of `blocks` blocks of WPB waves as the kernel runs it, the waves stepped in a shuffled
// order: a wave strides through its static rounds, then draws a ticket at the start of the body
// before the one that needs it (so it holds one ticket ahead), maps it to its list index when it
// needs it, and stops at the first "none".
struct Wave {
    int g, j;
    int li;         // the list index being worked on (before the first: one stride in front)
    bool dyn;       // past its static rounds
    int held;       // the ticket drawn ahead (-1: none)
    bool took;      // take() done, head() to come (other waves step in between)
    bool done;
};
static void test_walk(int count, int blocks, unsigned seed) {
    std::vector<int> taken(count > 0 ? count : 0, 0);
    int cursor[8] = {};
    GroupWalk gw[8];
    for (int g = 0; g < 8; ++g) gw[g] = group_walk(count, g, blocks);
    std::vector<Wave> w;
    for (int b = 0; b < blocks; ++b)
        for (int k = 0; k < WPB; ++k) {
            const int j = b / 8 * WPB + k;
            w.push_back(Wave{b & 7, j, gw[b & 7].begin + j - gw[b & 7].waves, false, -1, false, false});
        }
    int live = (int)w.size(), drawn_none = 0, unused = 0;
    auto static_left = [&](const Wave& x) { return !x.dyn && group_static_next(gw[x.g], x.li) != GROUP_NONE; };
    // GroupNext::take: the atomic, only once the static rounds are spent
    auto take = [&](Wave& x) {
        if (!static_left(x)) x.held = cursor[x.g]++;
    };
    // GroupNext::head: the next list index; a "none" reads nothing and ends the wave
    auto head = [&](Wave& x) {
        int li;
        if (static_left(x)) {
            li = group_static_next(gw[x.g], x.li);
            CHECK(li < gw[x.g].split);
        } else {
            x.dyn = true;
            CHECK(x.held >= 0);
            li = group_take(gw[x.g], x.held);
            x.held = -1;
            if (li == GROUP_NONE) ++drawn_none;
            else CHECK(li >= gw[x.g].split);
        }
        x.li = li;
        if (li == GROUP_NONE) {
            x.done = true;
            --live;
            return;
        }
        CHECK(li >= gw[x.g].begin && li < gw[x.g].end && li < count);
        if (li >= 0 && li < count) ++taken[li];
    };
    for (Wave& x : w) CHECK(group_static_first(gw[x.g], x.j) == group_static_next(gw[x.g], x.li));
    while (live > 0) {
        seed = seed * 1664525u + 1013904223u;
        Wave& x = w[(seed >> 8) % w.size()];
        if (x.done) continue;
        // a step: take (the wave's start, or a body's start), or the head() that follows it later
        if (!x.took) take(x);
        else head(x);
        x.took = !x.took;
    }
    for (const Wave& x : w) unused += x.held >= 0;
    for (int i = 0; i < count; ++i) CHECK(taken[i] == 1);
    // every wave stopped on a "none" of its own, the last ticket it drew, and holds no other: a
    // cursor ends at its ticket range plus its group's waves, far from overflow
    CHECK(drawn_none == (int)w.size() && unused == 0);
    for (int g = 0; g < 8; ++g) CHECK(cursor[g] == gw[g].end - gw[g].split + blocks / 8 * WPB);
}

int main() {
    test_plan();
    const int counts[] = {0, 1, 7, 8, 9, 4095, 4097, 20817};
    test_rule_literals();
    for (int count : counts)
        for (int blocks : {8, 1024}) {
            test_rule(count, blocks);
            for (unsigned seed : {1u, 2u, 12345u}) test_walk(count, blocks, seed);
        }
    if (failures) return 1;
    puts("group walk ok");
    return 0;
}
