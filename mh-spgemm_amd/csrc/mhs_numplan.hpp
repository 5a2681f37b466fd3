// mhs_numplan.hpp -- the numeric launch plan of a call, as a value.
//
// plan_numeric(h, sh) is the function launch-plan speculation rests on (see stats_same_plan in
// mhs_shape.hpp): which numeric kernels a call launches, in which order, with which grids, LDS
// sizes and row lists, from the Stats k_scan publishes and the call's shape.  It holds no pointer
// and no HIP type: issue_numeric (mhs_kernels.hip) turns one NumLaunch and the call's arrays into a
// kernel launch, run_numeric (mhs_api.cpp) deals the list over the streams.
// tests/numplan_check.cpp runs it on the host.
#pragma once
#include "mhs_groupwalk.hpp"
#include "mhs_shape.hpp"

namespace mhs {

// Block caps of the numeric launches (blocks; grids are multiples of 8: round8).
constexpr int MHS_NUM_WS_GRID = 4096;  // block cap of the small-row grouped numeric launch
constexpr int MHS_TINY64_GRID = 4096;  // block cap of the 64-lane tiny numeric launches (8192: wb-edu-like +6 %)
constexpr int MHS_NUM_W16H_GRID = 2048;  // block cap of the 10 KiB hash launch (4096: neutral at 16 KiB, profiles/r02za2_grid)
constexpr int MHS_COPY_CAP_BIG = 65536;  // the slot copy's block cap from 4 M rows (16384 below; delaunay-like -1 %, r05ab19)
constexpr int MHS_NUM_WSH_BIG = (1 << 21);  // small hash bins of at least this many rows: block cap MHS_NUM_WSH_BIG_GRID
constexpr int MHS_NUM_WSH_BIG_GRID = 65536;  // (cage15-like -2.5 % over 16384; 65536 for every bin: offshore-, webbase-like +1.5 %)
constexpr int MHS_NUM_WSX_GRID = 16384;  // ... of the small-row hash / direct launches (8192: cage15-like numeric +4.5 %, 4096: +13 %,
                                         // cant-perturbed +5 %; the grouped launch: 8192 measured +1.4 % on cant-like)
constexpr int MHS_DYN16_MAX = 32768;  // hash 10 KiB bins of at most this many rows: all rows from the cursor

// Dynamic LDS of a block-kernel launch: the header plus its largest row's tables, in
// 2 KiB steps, at most the bin's budget.
inline int block_lds(int need, int budget, int T) {
    if (need <= 0) return budget;
    const int b = (block_hdr(T) + need + 2047) & ~2047;
    return b < budget ? b : budget;
}
// A block bin runs as two launches when it holds rows on both sides of its LDS split.
inline bool block_split_on(const Stats& h, int k) {
    const int bin = k ? NUM_B1024 : NUM_B256;
    return h.num_block_big[k] > 0 && h.num_block_big[k] < h.num_count[bin];
}
// grouped bins: LDS regions of their largest group's need, 256-byte steps (k_scan's num_wave_need)
inline int wave_region(int need, int cap) {
    const int b = (need + 255) & ~255;
    return need <= 0 || b > cap ? cap : b;
}
inline int copy_lanes(int c) { return c == 0 ? 4 : c == 1 ? 8 : c == 2 ? 16 : 32; }

// The kernel families of the numeric phase.
enum NumKernel : int {
    NK_COPY,         // k_tiny_copy_rows<lanes>: numeric-first slot rows into C
    NK_COPY_HASH,    // k_copy_hash<lanes>: ... fused with the small hash wave bin
    NK_GLOBAL,       // k_num_block<1024, global>
    NK_BLOCK1024,    // k_num_block<1024>
    NK_BLOCK256,     // k_num_block<256>
    NK_HASH16,       // k_num_wave_hash<10 KiB>
    NK_HASH,         // k_num_wave_hash<5 KiB>
    NK_DIRECT16,     // k_num_wave_direct<10 KiB>
    NK_DIRECT,       // k_num_wave_direct<5 KiB>
    NK_GROUP16,      // k_num_wave<10 KiB, grouped>: NUM_W16G
    NK_GROUP,        // k_num_wave<10 KiB, grouped>: NUM_WSG (regions of wave_bytes)
    NK_TINY64,       // k_tiny_num<64, K of the class>
    NK_TINY_SMALL,   // k_tiny_num_small: tiny classes 0..3 in one launch
};

// The 32-lane-or-narrower numeric tiny classes in one launch: class c[k] takes blocks
// [blk0[k], blk0[k+1]) (multiples of 8 keep the XCD walk).  The slot copy lists its classes
// here too, without block ranges: it walks A's rows in row order.
struct TinyFused {
    int nclass;
    int c[4];
    int count[4];
    int blk0[5];
};

enum : int { LIST_SPLIT = 0, LIST_CLASSES = -1 };
// One launch.  Every field is an int (no padding: plans compare bytewise).
struct NumLaunch {
    int kernel;       // NumKernel
    int variant;      // its integer template choice: copy lanes (4 / 8 / 16), tiny class (NK_TINY64)
    int grid, block, lds;  // blocks, threads, dynamic LDS bytes
    int list_bin;     // the rows: bin list_bin's list; LIST_SPLIT: split_list + list_off; LIST_CLASSES:
    int list_off;     // the bin lists of `fused`'s classes
    int count, slot;  // rows, cursor slot
    int wave_bytes;   // grouped wave bins: LDS bytes per wave
    int gbytes;       // global bin: scratch bytes per block
    int qall;         // 10 KiB hash bin: every row from the cursor
    int hash_blocks;  // NK_COPY_HASH: the leading blocks that walk the hash rows
    int after_split;  // reads split_list: waits for the split event (off the call's stream)
    TinyFused fused;
    int cursor_walk;  // grouped wave bins: about the resident set of waves, groups from the row cursors (mhs_groupwalk.hpp)
};

constexpr int NUM_PLAN_MAX = 16;  // (at most 14: copy or fused tiny, global, 2 x 2 block, 9 wave / tiny bins)
struct NumPlan {
    int n;
    int o32;  // 32-bit byte offsets for the B gathers (every launch's template choice)
    NumLaunch launch[NUM_PLAN_MAX];
};

// What plan_numeric reads besides the Stats.
struct NumShape {
    int M, nnzA, nnzB;
    int bx_on;        // the value walks read B's arrays extended by the near union rows
    int slot_rows;    // numeric-first: tiny classes 0..3 hold slot rows (copied, not computed)
    int split;        // k_split_bins partitioned the splittable block bins' lists
    int global_grid;  // block cap of the global bin
    int cus = 0;        // compute units (0: not known -- the grouped bins keep their static walk)
    int group_cap = 0;  // MHS_OPT_GROUP_GRID: block cap of the grouped cursor walk (0: the resident set)
    int no_o32 = 0;     // MHS_NO_O32=1 (tests): 64-bit byte offsets whatever the sizes
};

// Numeric launches of the non-empty bins, largest rows first: dealt round-robin over the streams
// (stream_of), one bin's tail overlaps the next bin's bulk (the reference runs its bins on 12
// streams, src/Tool.cu:6-10).
// Measured (round 4, profiles/r04): dealing by estimated work (LPT over products and the heaviest
// row) put the hub rows' launch behind the bulk bins -- wb-edu-like +3 %, webbase-like +3 % --
// concurrent launches share the CUs, and the hub rows' 1024-thread blocks, one per CU for their
// LDS, progress only as CUs free up; started first, they hold their CUs from the start.
// Stats fields read: num_count, num_global_need, num_block_need, num_block_small_need,
// num_block_big, num_wave_need -- all among those stats_same_plan compares.
inline NumPlan plan_numeric(const Stats& h, const NumShape& sh) {
    NumPlan p{};
    // 32-bit byte offsets for the B gathers when B's value array (extended by the union rows)
    // stays below 4 GiB: nnz(B) + 3 nnz(A) < 2^29 (the reference's int32 CSR allows up to 2^31)
    p.o32 = !sh.no_o32 && (long long)sh.nnzB + (sh.bx_on ? 3LL * sh.nnzA : 0) < (1LL << 29);
    // a launch over `bin`'s list (cursor slot = bin) of `blocks` blocks at most `cap`
    auto add = [&](int kernel, int bin, int count, long long blocks, int cap, int threads, int lds) -> NumLaunch& {
        NumLaunch& l = p.launch[p.n < NUM_PLAN_MAX ? p.n++ : NUM_PLAN_MAX - 1];
        l = NumLaunch{};
        l.kernel = kernel;
        l.grid = round8(blocks, cap);
        l.block = threads;
        l.lds = lds;
        l.list_bin = bin;
        l.count = count;
        l.slot = bin > 0 ? bin : 0;
        return l;
    };
    auto wave_bin = [&](int kernel, int bin, int cap, int wave_bytes) -> NumLaunch& {
        const int count = h.num_count[bin];
        return add(kernel, bin, count, (count + WPB - 1) / WPB, cap, 256, WPB * wave_bytes);
    };
    // class c of the tiny classes 0..3, largest first, `lanes` lanes a row: blocks of its own in f
    auto fused = [&](bool ranges, int lanes(int)) {
        TinyFused f{};
        for (int c = 3; c >= 0; --c) {
            const int count = h.num_count[NUM_TINY + c];
            if (count <= 0) continue;
            const int per = 256 / lanes(c);
            f.c[f.nclass] = c;
            f.count[f.nclass] = count;
            if (ranges) f.blk0[f.nclass + 1] = f.blk0[f.nclass] + round8((count + per - 1) / per, 4096);
            ++f.nclass;
        }
        return f;
    };
    const int wsh_cap = h.num_count[NUM_WSH] >= MHS_NUM_WSH_BIG ? MHS_NUM_WSH_BIG_GRID : MHS_NUM_WSX_GRID;

    // Numeric-first rows: their copy of the slot values into C (short and HBM-bound),
    // ... fused with the small hash wave bin when those two are the whole phase (k_copy_hash)
    // (r06fc: mac_econ-like numeric 45 -> 34 us, pipelined step -5 %)
    bool fuse = false;
    if (sh.slot_rows) {
        const TinyFused f = fused(false, copy_lanes);
        fuse = f.nclass > 0 && h.num_count[NUM_WSH] > 0;
        for (int b = 1; b < NUM_NB && fuse; ++b)
            fuse = b == NUM_WSH || (b >= NUM_TINY && b < NUM_TINY + 4) || h.num_count[b] <= 0;
        int ncopy = 0, cmed = 0;
        for (int k = 0; k < f.nclass; ++k) ncopy += f.count[k];
        for (int c = 0, acc = 0; c < 4; ++c) {  // the class of the median slot row
            acc += h.num_count[NUM_TINY + c];
            if (2 * acc >= ncopy) {
                cmed = c;
                break;
            }
        }
        if (f.nclass > 0) {
            // lanes per row by the median row's class
            const int Lw = copy_lanes(cmed) > 16 ? 16 : copy_lanes(cmed);
            const int grid = round8((sh.M + 256 / Lw - 1) / (256 / Lw), sh.M >= MHS_NFT_BIG_M ? MHS_COPY_CAP_BIG : 16384);
            NumLaunch& l = fuse ? wave_bin(NK_COPY_HASH, NUM_WSH, wsh_cap, NUM_WS_BYTES)
                                : add(NK_COPY, LIST_CLASSES, ncopy, grid, grid, 256, 0);
            if (fuse) {  // the hash rows' blocks first, then the copy's
                l.hash_blocks = l.grid;
                l.grid += grid;
            }
            l.variant = Lw;
            l.fused = f;
        }
    }
    if (h.num_count[NUM_GLOBAL] > 0) {
        const int count = h.num_count[NUM_GLOBAL];
        NumLaunch& l = add(NK_GLOBAL, NUM_GLOBAL, count, 0, 0, 1024, BLOCK_HDR_1024);
        l.grid = count < sh.global_grid ? count : sh.global_grid;
        l.gbytes = (int)align16(h.num_global_need);
    }
    // block bins: rows past the bin's LDS split (hub rows) in a launch of their own, so the
    // others run at the occupancy their own tables allow
    auto block_bin = [&](int kernel, int bin, int k, int T, int grid_cap, int budget, int big_slot) {
        const int count = h.num_count[bin];
        if (count <= 0) return;
        if (sh.split && block_split_on(h, k)) {  // k_split_bins: small rows first, hub rows last
            const int big = h.num_block_big[k];
            const int off = k ? 0 : (h.num_count[NUM_B1024] > 0 ? h.num_count[NUM_B1024] : 0);
            NumLaunch& hub = add(kernel, LIST_SPLIT, big, big, grid_cap, T, block_lds(h.num_block_need[k], budget, T));
            hub.list_off = off + (count - big);
            hub.slot = big_slot;
            hub.after_split = 1;
            NumLaunch& rest = add(kernel, LIST_SPLIT, count - big, count - big, grid_cap, T,
                                  block_lds(h.num_block_small_need[k], budget, T));
            rest.list_off = off;
            rest.slot = bin;
            rest.after_split = 1;
        } else {
            add(kernel, bin, count, count, grid_cap, T, block_lds(h.num_block_need[k], budget, T));
        }
    };
    block_bin(NK_BLOCK1024, NUM_B1024, 1, 1024, 256, LDS_MAX - 1024, BLOCK_BIG_SLOT + 1);
    block_bin(NK_BLOCK256, NUM_B256, 0, 256, 1024, NUM_B256_BYTES, BLOCK_BIG_SLOT);
    if (h.num_count[NUM_W16H] > 0)  // (few rows per resident wave: the launch's end is one heavy row)
        wave_bin(NK_HASH16, NUM_W16H, MHS_NUM_W16H_GRID, NUM_W16_BYTES).qall = h.num_count[NUM_W16H] <= MHS_DYN16_MAX;
    if (h.num_count[NUM_WSH] > 0 && !fuse) wave_bin(NK_HASH, NUM_WSH, wsh_cap, NUM_WS_BYTES);
    if (h.num_count[NUM_W16] > 0) wave_bin(NK_DIRECT16, NUM_W16, 2048, NUM_W16_BYTES);
    for (int c = TINY_NC - 1; c >= 4; --c) {  // 64-lane classes: kernels of their own (registers)
        const int count = h.num_count[NUM_TINY + c];
        if (count <= 0) continue;
        const int per = 256 / tiny_w(c);
        add(NK_TINY64, NUM_TINY + c, count, (count + per - 1) / per, MHS_TINY64_GRID, 256, 256 * tiny_k(c) * 8).variant = c;
    }
    static_assert(tiny_w(3) <= 32 && tiny_k(0) <= TINY_FUSED_KMAX && tiny_k(1) <= TINY_FUSED_KMAX &&
                      tiny_k(2) <= TINY_FUSED_KMAX && tiny_k(3) <= TINY_FUSED_KMAX && tiny_w(4) == 64,
                  "classes 0..3 fuse (W <= 32, K <= TINY_FUSED_KMAX)");
    if (!sh.slot_rows) {  // (numeric-first: copied above)
        const TinyFused f = fused(true, [](int c) { return tiny_w(c); });
        if (f.nclass > 0) {
            int rows = 0;
            for (int k = 0; k < f.nclass; ++k) rows += f.count[k];
            const int blocks = f.blk0[f.nclass];
            add(NK_TINY_SMALL, LIST_CLASSES, rows, blocks, blocks, 256, 256 * TINY_FUSED_KMAX * 8).fused = f;
        }
    }
    if (h.num_count[NUM_W16G] > 0) {
        const int wb = wave_region(h.num_wave_need[1], NUM_W16_BYTES);
        wave_bin(NK_GROUP16, NUM_W16G, 2048, wb).wave_bytes = wb;
    }
    if (h.num_count[NUM_WSG] > 0) {
        const int wb = wave_region(h.num_wave_need[0], NUM_WSG_BYTES);
        NumLaunch& l = wave_bin(NK_GROUP, NUM_WSG, MHS_NUM_WS_GRID, wb);
        l.wave_bytes = wb;
        // More groups than the resident waves can take one each: launch the resident set and let
        // every wave loop -- static rounds, the last full round and the partial one drawn from the
        // XCD group's cursor (mhs_groupwalk.hpp).  (A block of the static grid lives for one or
        // two groups: each wave pays its launch and the dependent round trips before its first
        // body, and a block's LDS frees only with its slowest wave.)  Smaller bins keep the
        // static grid: a wave a group.  Measured on cant-like (20,817 groups, 256 CUs): the kernel
        // 165.0 -> 161.3 us, waves resident in 83 -> 88 % of the slot-time; every group from the
        // cursor: +8 %; no round from the cursor: +5 %; 2048 blocks: +5 %.
        const int resident = sh.group_cap > 0 ? sh.group_cap : sh.cus > 0 ? group_resident_blocks(sh.cus, wb) : 0;
        const int blocks = (l.count + WPB - 1) / WPB;
        if (resident > 0 && (blocks > resident || sh.group_cap > 0)) {
            l.grid = round8(blocks, resident < MHS_NUM_WS_GRID ? resident : MHS_NUM_WS_GRID);
            l.cursor_walk = 1;
        }
    }
    if (h.num_count[NUM_WS] > 0) wave_bin(NK_DIRECT, NUM_WS, MHS_NUM_WSX_GRID, NUM_WS_BYTES);
    return p;
}

// Numeric launches a call makes for these bin counts, as numeric_streams counts them (the
// 32-lane tiny classes share one; a splittable block bin counts two).  An upper estimate of the
// plan's length, not its definition: the plan is one shorter where the slot copy fuses with the
// small hash bin, and one shorter per splittable block bin whose split was not taken (one stream,
// or below the split's product threshold).  The stream count depends on this exact rule.
inline int numeric_launches(const Stats& h) {
    int n = 0, small = 0;
    for (int b = 1; b < NUM_NB; ++b) {
        if (h.num_count[b] <= 0) continue;
        if (b >= NUM_TINY && b < NUM_TINY + 4) small = 1;
        else ++n;
    }
    return n + small + block_split_on(h, 0) + block_split_on(h, 1);
}

// The dealing rule: launch i of a plan dealt over n streams goes to stream i % n -- the first
// (largest rows) on the call's stream at once, and the last, bulk wave bins tend to stay there.
inline int stream_of(int i, int n) { return n > 1 ? i % n : 0; }

}  // namespace mhs
