// mhs_frontplan.hpp -- the launches of a call before its numeric phase, as a value.
//
// Which kernels go out between the start of a call and k_scan, with which template variants, grids,
// LDS and streams, and what a speculated plan leaves out: plan_front_rows (the mask of B, the row
// analysis, the bin lists), plan_front_symbolic (the symbolic bins, the near check) and front_scan.
// Two stages, because the numeric-first probe hands k_analyze's counts to the host between them:
// nft and sym_big are known only then.  No pointer and no HIP type: issue_front (mhs_kernels.hip)
// turns one FrontLaunch and the call's arrays into a kernel launch, mhs_api.cpp walks the plans and
// keeps the streams, events and hand-offs.  tests/frontplan_check.cpp runs all of it on the host.
#pragma once
#include "mhs_shape.hpp"

namespace mhs {

// Rows per block of the row_ptr scan and the bin lists: 4096 (four per thread) for big
// matrices -- a quarter of the blocks, so a quarter of the per-(block, bin) cursor atomics
// (tiny-row matrices of millions of rows were bound by them) -- 1024 below, where fewer
// blocks would leave the chip idle (measured: cant-like -6% at 4096).
constexpr int MHS_SCAN_BIG_M = (1 << 19);
constexpr int MHS_MASK_GMAX = 64;  // k_mask_b: from 8 lanes per row up to the whole wave
constexpr int MHS_AN_GMAX = 8;  // k_analyze: 8 lanes per row (several rows per wave overlap their load chains)
constexpr int MHS_LANE_AVG = 9;  // k_mask_b / k_analyze: a lane per row below this many entries a row on average
constexpr int MHS_SYM_WAVE_GRID = 2048;  // block cap of k_sym_common's wave rows (65536: cage15-like -3 %, cop20k-, webbase-, mac_econ-like +5 %)
constexpr int MHS_SYM_WAVE_GRID_BIG = 65536;  // ... when the probe counted >= 2^21 table rows (FrontShape::sym_big)
// block cap of each numeric-first symbolic tiny class: 4096, 16384 from 4 M rows (r05ab17/18:
// delaunay-like 10.26 -> 9.70 ms, GAP-road-like 4.53 -> 4.43 at 16384, but mac_econ-, scircuit-like
// +5-6 %; 512-2048 slower on every huge matrix, delaunay-like up to 19 ms)
constexpr int MHS_NFT_GRID = 4096, MHS_NFT_GRID_BIG = 16384;  // (from MHS_NFT_BIG_M rows)
constexpr int MHS_SYM_B256_GRID = 1024;  // block cap of the persistent 256-thread symbolic bin launch
constexpr int MHS_NEAR_GRID = 2048;  // k_near's block cap
// Tiny symbolic rows without slots: blocks [TINY_SYM_GRID*c, TINY_SYM_GRID*(c+1)) of the tiny role walk
// class c's list.  With slots (numeric-first) it is class 4's fixed grid.
constexpr int TINY_SYM_GRID = 1024;

// The kernel families, in the order a call launches them.
enum FrontKernel : int {
    FK_MASK_LANE,     // k_mask_lane<variant>: a lane per B row, `variant` entries a load
    FK_MASK,          // k_mask_b<variant, 4>: `variant` lanes per B row, four chunks a round trip
    FK_ANALYZE_LANE,  // k_analyze_lane<variant>
    FK_ANALYZE,       // k_analyze<variant, 4>: `variant` lanes per A row, four entries a lane
    FK_PROBE_PUBLISH, // k_probe_publish: the numeric-first probe's counts to the host
    FK_BIN_LIST,      // k_bin_list<variant>: `variant` rows per thread
    FK_SYM_COMMON,    // k_sym_common: the small-table wave bin and every tiny class
    FK_SYM_RARE,      // k_sym_rare: 10 KiB waves, the 157 KiB block bin, global memory (+ the near check)
    FK_SYM_B256,      // k_sym_block<256>: the 32 KiB block bin
    FK_NEAR,          // k_near: the near check in a launch of its own
    FK_SCAN,          // k_scan<variant>
};
enum : int { FRONT_CALL = 0, FRONT_AUX = 1 };  // FrontLaunch::stream: the call's stream, the first aux stream

// One launch.  Every field is an int (no padding: plans compare bytewise).
struct FrontLaunch {
    int kernel;            // FrontKernel
    int variant;           // its integer template choice
    int grid, block, lds;  // blocks, threads, dynamic LDS bytes
    int words;             // k_analyze's per-block words (FK_ANALYZE*: written, FK_PROBE_PUBLISH: summed)
    int stream;            // FRONT_CALL / FRONT_AUX
    int after_join;        // a forked pass: goes out once the aux stream has joined the call's
    int wave_blocks;       // k_sym_common: the leading blocks that walk the wave bin
    int blk0[TINY_SYMX_NC + 1];  // ... numeric-first: tiny class c takes blocks [blk0[c], blk0[c+1]) after them
    int with_near;         // k_sym_rare: its phase 0 checks the near row-group candidates
};

constexpr int FRONT_PLAN_MAX = 4;
struct FrontPlan {
    int n;
    int fork;      // FRONT_AUX launches run beside the call's stream: fork before the first launch, join
                   // before the first after_join launch (or behind the last launch)
    int left_out;  // launches a speculated plan proved empty (MHS_STAT_SPEC_SKIPPED)
    FrontLaunch launch[FRONT_PLAN_MAX];
};
inline FrontLaunch& push(FrontPlan& p, const FrontLaunch& l) {
    return p.launch[p.n < FRONT_PLAN_MAX ? p.n++ : FRONT_PLAN_MAX - 1] = l;
}

// What the plans read besides a speculated call's Stats.
struct FrontShape {
    int M, MB;       // rows of A (of this pass), of B
    int nnzA, nnzB;  // (a row chunk: A's share by rows -- it only steers geometry)
    int mask;        // this pass masks B (a chunked call: its first chunk)
    int probe;       // the numeric-first probe: k_analyze's counts go to the host before the bin lists
    int nft;         // numeric-first tiny rows with value slots (after the probe)
    int sym_big;     // the probe counted >= 2^21 rows past the tiny classes
    int near;        // near row groups are planned
    int fork;        // the rare symbolic bins run on the aux stream
};

// The lane kernels take every matrix below MHS_LANE_AVG = 9 entries a row, so a lane group never starts
// below 8 lanes, its rows average more than its width (four chunks a round trip, always), and k_analyze's
// group is MHS_AN_GMAX wide: the narrower groups and the one-chunk variants of both kernels (2-lane
// groups had measured -3.6 % on GAP-road-like before the lane kernels) are not built any more.
// tests/frontplan_check.cpp sweeps the rules for the variants they reach: those issue_front instantiates.
static_assert(MHS_LANE_AVG > MHS_AN_GMAX && MHS_AN_GMAX == 8, "no group below 8 lanes, rows longer than the group");

// k_mask_b / k_mask_lane: about four chunk iterations per row -- a wave then holds several rows, whose
// dependent load chains overlap (measured on gfx950: 64-lane rows were latency-bound).
inline FrontLaunch mask_launch(long long nnzB, int MB) {
    const long long avg = MB > 0 ? nnzB / MB : 0;
    if (avg < MHS_LANE_AVG) return {FK_MASK_LANE, avg < 4 ? 4 : 8, (MB + 255) / 256, 256};  // short rows: a lane per row
    // (round 6: groups widen from rows of 16 G entries on, not 8 G -- eight rows a wave for
    // cant-like's 69-entry rows, three chunk rounds instead of two: the waves overlap their
    // ptr -> col chains, cant-like pipelined steps -1.5 %, cant-perturbed-like -0.6 %)
    int G = 8;
    while (2 * G <= avg / 8 && G < MHS_MASK_GMAX) G <<= 1;
    return {FK_MASK, G, (MB + 256 / G - 1) / (256 / G), 256};
}
// k_analyze: MHS_AN_GMAX lanes per row, four entries a lane; k_analyze_lane: a lane per row, two per-block
// words (128 rows each).  The workspace (the per-block words), make_work and the launch all ask here.
inline FrontLaunch analyze_launch(long long nnzA, int M) {
    const long long avg = M > 0 ? nnzA / M : 0;
    const int lane = (M + 255) / 256, group = (M + 256 / MHS_AN_GMAX - 1) / (256 / MHS_AN_GMAX);
    if (avg < MHS_LANE_AVG) return {FK_ANALYZE_LANE, avg < 4 ? 4 : 8, lane, 256, 0, 2 * lane};
    return {FK_ANALYZE, MHS_AN_GMAX, group, 256, 0, group};
}
inline int scan_per(int M) { return M >= MHS_SCAN_BIG_M ? 4 : 1; }  // rows per thread of k_bin_list / k_scan

// Stage 1: the mask of B, the row analysis and the symbolic bin lists.  With the probe the host
// decides nft / sym_big after FK_PROBE_PUBLISH (k_bin_list's grid does not depend on them).
// The mask runs on every call, even when B is unchanged: it rewrites all of bmeta, and k_scan
// marks near heads in bmeta.w (over the lo tile) for the numeric pass -- a skipped mask pass
// would let stale NEAR_HEAD bits reach k_analyze.
inline FrontPlan plan_front_rows(const FrontShape& sh) {
    FrontPlan p{};
    if (sh.mask && sh.MB > 0) push(p, mask_launch(sh.nnzB, sh.MB));
    if (sh.M <= 0) return p;
    const int words = push(p, analyze_launch(sh.nnzA, sh.M)).words;
    if (sh.probe) push(p, {FK_PROBE_PUBLISH, 0, 64, 1024, 0, words});
    const int per = scan_per(sh.M);
    push(p, {FK_BIN_LIST, per, (sh.M + 1024 * per - 1) / (1024 * per), 1024});
    return p;
}

// Stage 2: the symbolic bins -- persistent grids that read their bins' sizes on the device -- and the
// near check.  One order: k_sym_common on the call's stream; the rare bins behind it, or (sh.fork)
// beside it on the aux stream -- rows of the rare bins are long and few, their tail no longer idles
// the chip; the 256-thread bin on the call's stream (at one block per CU in k_sym_rare it would hold a
// fifth of the rows in flight; webbase-like: 60 us off the symbolic phase beside k_sym_rare); forked,
// the join and then k_near, which k_sym_rare runs itself when it follows k_sym_common on one stream.
// `spec` (the previous call's Stats, a speculated call) gives the bins' sizes ahead of the device.
// The roles of k_sym_common are sized to them: an empty role launches no blocks.  Unforked, the rare
// bins' launch is left out when its bins and the near candidates are empty, the 256-thread bin's
// when that bin is.  A row in a bin the plan had empty changes the Stats: k_scan rejects the plan and
// the call reruns unspeculated, every role's grid sized for M rows, its surplus blocks gone after
// one load.  (r06pg: mac_econ-like -2 %, scircuit-like -3 %, webbase-like -0.6 %: thousands of empty
// blocks no longer dispatched.)  Stats fields read: sym_count, near_heads -- stats_same_plan compares both.
inline FrontPlan plan_front_symbolic(const FrontShape& sh, const Stats* spec) {
    FrontPlan p{};
    p.fork = sh.fork;
    const int M = sh.M;
    if (M <= 0) return p;
    auto rows_of = [&](int bin) { return spec ? spec->sym_count[bin] : M; };
    // (sym_big: table rows, nearly all in the wave bin -- the numeric hash bin's big-grid rule;
    // r06i: cage15-like -3.2 %; wb-edu-like, 1.9 M such rows, keeps 2048)
    const int wave_blocks = rows_of(SYM_WAVE) == 0 ? 0
        : round8((rows_of(SYM_WAVE) + WPB - 1) / WPB, sh.sym_big ? MHS_SYM_WAVE_GRID_BIG : MHS_SYM_WAVE_GRID);
    constexpr int NCL = MHS_SYM_SORT64 ? TINY_SYMX_NC : TINY_SYM_NC;
    int blk0[TINY_SYMX_NC + 1] = {};
    int tiny_blocks = TINY_SYM_GRID * NCL;
    if (sh.nft) {  // (the classes' sizes are on the device: grids for M rows each, as numeric's)
        for (int c = 0; c < TINY_SYM_NC; ++c) {
            const int per = 256 / tiny_w(c), rows = rows_of(SYM_TINY + c);
            blk0[c + 1] = blk0[c] + (rows == 0 ? 0 : round8((rows + per - 1) / per, M >= MHS_NFT_BIG_M ? MHS_NFT_GRID_BIG : MHS_NFT_GRID));
        }
        const bool c4 = MHS_SYM_SORT64 && rows_of(SYM_TINY + 4) > 0;
        blk0[TINY_SYMX_NC] = blk0[TINY_SYM_NC] + (c4 ? TINY_SYM_GRID : 0);  // class 4: a walk
        tiny_blocks = blk0[TINY_SYMX_NC];
    } else if (spec) {  // (class c's blocks are [1024 c, 1024 (c+1)): all of them, or none)
        int rows = 0;
        for (int c = 0; c < NCL; ++c) rows += spec->sym_count[SYM_TINY + c];
        if (rows == 0) tiny_blocks = 0;
    }
    if (wave_blocks + tiny_blocks > 0) {
        FrontLaunch& l = push(p, {FK_SYM_COMMON, 0, wave_blocks + tiny_blocks, 256, WPB * SYM_WAVE_BYTES});
        l.wave_blocks = wave_blocks;
        for (int c = 0; c <= TINY_SYMX_NC; ++c) l.blk0[c] = blk0[c];
    }
    const bool near_on = sh.near && M > 1 && !sh.nft;
    const bool trim = spec && !sh.fork;  // (a forked pass leaves no launch out)
    const bool rare = !trim || spec->sym_count[SYM_WM] > 0 || spec->sym_count[SYM_B1024] > 0 ||
                      spec->sym_count[SYM_GLOBAL] > 0 || (sh.near && spec->near_heads > 0);
    const bool b256 = !trim || spec->sym_count[SYM_B256] > 0;
    if (rare) {
        FrontLaunch& l = push(p, {FK_SYM_RARE, 0, 256, 1024, LDS_MAX - 1024});
        l.stream = sh.fork ? FRONT_AUX : FRONT_CALL;
        l.with_near = near_on && !sh.fork;
    }
    if (b256) push(p, {FK_SYM_B256, 0, round8(M, MHS_SYM_B256_GRID), 256, SYM_B256_BYTES});
    p.left_out = !rare + !b256;
    // a persistent grid over the device-side candidate count (none: the waves return at once)
    if (near_on && sh.fork) push(p, {FK_NEAR, 0, round8((M / 3 + WPB - 1) / WPB, MHS_NEAR_GRID), 256}).after_join = 1;
    return p;
}

// k_scan: row_ptr and the numeric bins, behind every symbolic launch on the call's stream
// (its state words were zeroed by k_analyze: SCAN_ITEMS-row blocks, enough for either width).
inline FrontLaunch front_scan(int M) {
    const int per = scan_per(M);
    return {FK_SCAN, per, (M + 1 + 1024 * per - 1) / (1024 * per), 1024};
}

}  // namespace mhs
