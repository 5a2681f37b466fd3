// mhs_valplan.hpp -- values-only SpGEMM (mhs_spgemm_values): row classes and the launch plan, as data.
//
// A values plan recomputes C.val on a kept pattern: every row of C is told its sorted columns and
// only has to find each product's slot.  How a row finds it is its class, a function of the row's
// C length n, its C column span (last - first + 1) and its product count:
//
//   VC_NONE          n == 0: nothing to compute
//   VC_TEAM          short rows: a team of VAL_TEAM_LANES lanes per row, 8 rows per wave64; the row's
//                    columns staged in the team's LDS slice, slot by binary search, FP64 sums beside them
//   VC_WAVE_DIRECT   one wave64 per row, span-indexed sums acc[col - first] in the wave's LDS slice:
//   VC_BLOCK_DIRECT  ... or one block per row with up to the whole 160 KiB.  No search; the sums are
//                    gathered through C.col afterwards
//   VC_WAVE_SEARCH   span too wide: the row's C.col staged in LDS once, slot by binary search,
//   VC_BLOCK_SEARCH  position-indexed sums (12 bytes per C entry)
//   VC_GLOBAL        rows past one workgroup's 160 KiB (and long rows without products): the row's
//                    Cval segment zeroed, C.col searched in HBM, sums by HBM atomics
// Those are the product-form classes: they walk every product of the row.  A masked plan
// (mhs_values_plan_create_masked: C's pattern may be smaller than the product's) has one more:
//   VC_DOT           inner-product form: a lane per mask entry (i, j) searches each of the row's A
//                    columns in B^T's row j.  No LDS sums, no atomics; val_class_masked picks it.
//
// LDS arithmetic (gfx950: 160 KiB per CU and per workgroup, 32 waves per CU):
//   team    12 B x n <= 768 B per row, 32 rows per 256-thread block: <= 24 KiB, 6 blocks per CU
//   wave    VAL_WAVE_BYTES = 8 KiB per wave, 4 waves per block: span <= 1024 direct, n <= 682 searched;
//           at the cap 4 blocks (16 waves) per CU
//   block   VAL_BLOCK_BYTES = 159,744: span <= 19,968 direct, n <= 13,312 searched
//   The wave and block kernels also hold a stage of A entries in static LDS (walk_staged): 1 KiB per
//   wave, 4 KiB (VAL_STAGE_BYTES) per block -- what the block classes' dynamic LDS leaves of the 160 KiB.
// A launch declares what its class's largest row needs (ValCounts::need, k_val_classify's maximum),
// not the cap, so banded matrices run at the occupancy their own spans allow.
//
// The value type.  A plan has one, FP64 or FP32, and everything above that is bytes is a function of its
// size vb (8 or 4; the names without a vb argument are the FP64 figures).  FP32: a direct sum is 4 B, a
// searched entry 8 B (sum, then column), so
//   team    8 B x n <= 512 B per row
//   wave    span <= 2048 direct, n <= 1024 searched
//   block   span <= 39,936 direct, n <= 19,968 searched
// and rows move to cheaper classes.  Counts are not bytes and do not move: VAL_TEAM_NMAX, the product caps,
// VAL_DENSE_RATIO, VAL_BLOCK_SMALL, VAL_GROUP, the grid caps.  val_slice_entries / val_slice_fits are the
// guards of a row's LDS slice, for the kernels' row frame (mhs_valwalk.hpp) and for the host alike.
//
// The width.  A plan has a third fixed property, its width W (1, 2 or 4: VAL_WIDTH_MAX): the value sets one walk
// of the pattern accumulates (mhs_values_plan_create_batched).  With it everything above that is bytes depends on
// the sum bytes sb = W x vb, 4 / 8 / 16 / 32: a direct column costs sb, a searched entry sb + 4 (W sums and the one
// shared column), and every function below that takes vb serves sb.  W = 1 is the tables above; FP32 W = 2 is the
// FP64 table (sb = 8); further
//   sb  plans                wave-direct span  wave-search n  block-direct span  block-search n  team row
//   16  FP64 W=2, FP32 W=4                512            408              9,984           7,986   1,280 B
//   32  FP64 W=4                          256            226              4,992           4,436   2,304 B
// A mixed plan (FP32 values, FP64 sums: ValAccum below) of width W has the rows of the FP64 plan of width W: sb = 8 W.
// A slice holds its sums set-major: acc[w x pitch + slot], pitch the span (direct) or the slice's entry count
// (search), the one column array behind all W planes.  Counts still do not move.  At sb = 32 the team launch at its
// cap is 73,728 B, past the VAL_LDS_PLAIN a launch may take unasked: val_team_registers says which team kernels
// init_values_attributes registers for val_team_launch_cap (the forward's and the backward's alike).  plan_grad takes
// sb too: a wide plan's backward holds W cotangents per C entry where the forward holds W sums
// (mhs_spgemm_values_grad_batched).
//
// plan_values(counts) is the whole launch plan of a hot call; issue_values (mhs_values.hip) turns one
// ValLaunch and the call's arrays into a kernel launch.  No pointer and no HIP type in here:
// tests/valplan_check.cpp runs it on the host.  plan_grad(counts) is the launch plan of the backward
// (mhs_spgemm_values_grad and _grad_batched; issue_values_grad, mhs_values_grad.hip): tests/gradplan_check.cpp and
// tests/gradplan_batched_check.cpp.
#pragma once
#include "mhs_shape.hpp"

namespace mhs {

enum ValClass : int {
    VC_NONE = 0,
    VC_TEAM = 1,
    VC_WAVE_DIRECT = 2,
    VC_WAVE_SEARCH = 3,
    VC_BLOCK_DIRECT = 4,
    VC_BLOCK_SEARCH = 5,
    VC_GLOBAL = 6,
    VC_COUNT = 7,  // the count of product-form classes (what val_class returns is below it)
    VC_DOT = 7,    // the masked plans' dot class: the last index of mhs_values_info::rows
};
constexpr int VAL_NCLASS = 8;  // capacity of the per-class arrays (mhs_values_info::rows)

constexpr int VAL_TEAM_LANES = 8;      // lanes per team row
constexpr int VAL_TEAM_ROWS = 256 / VAL_TEAM_LANES;  // rows per 256-thread block
constexpr int VAL_TEAM_NMAX = 64;      // C entries of a team row (6 search steps)
constexpr int VAL_TEAM_PMAX = 512;     // products of a team row (64 per lane)
constexpr int VAL_WAVE_BYTES = 8192;   // LDS per wave of the wave classes
constexpr int VAL_WAVE_PMAX = 2048;    // products of a wave row (32 per lane, half a team lane's 64); past it a block's 4x lanes
constexpr int VAL_STAGE = 256;          // A entries a block stages at a time (16 B each, static LDS)
constexpr int VAL_STAGE_BYTES = VAL_STAGE * 16;
constexpr int VAL_BLOCK_BYTES = LDS_MAX_C - VAL_STAGE_BYTES;  // dynamic LDS of the block classes
constexpr int VAL_DENSE_RATIO = 16;    // span <= 16 n: zeroing and gathering the span costs less than searching
constexpr int VAL_BLOCK_SMALL = 32768; // block launches of at most this much LDS run 256 threads, else 1024
constexpr int VAL_GROUP = 16;          // lanes that share one A entry in the wave / block / global walks
// Masked AUTO: a row goes to the dot class when VAL_DOT_RATIO x its dot form's search steps < its products
// (a search step is a dependent HBM / L2 load, a product a streamed one: DESIGN section 11 has the sweep)
constexpr int VAL_DOT_RATIO = 2;

// Bytes of a value: vb, 8 (FP64) or 4 (FP32)
constexpr int VAL_VB_F64 = 8, VAL_VB_F32 = 4;
__host__ __device__ constexpr bool val_vb_ok(int vb) { return vb == VAL_VB_F64 || vb == VAL_VB_F32; }
// The width of a plan, W: the value sets one walk accumulates; and the sum bytes sb = W x vb that stand wherever
// a function below takes vb (W = 1: sb = vb)
constexpr int VAL_WIDTH_MAX = 4;
__host__ __device__ constexpr bool val_width_ok(int w) { return w == 1 || w == 2 || w == 4; }
__host__ __device__ constexpr bool val_sb_ok(int sb) { return sb == 4 || sb == 8 || sb == 16 || sb == 32; }
__host__ __device__ constexpr int val_search_entry(int vb) { return vb + 4; }  // a searched entry: its sum(s) and its column

// The sum type of a plan, its fifth fixed property (mhs_accum of the C ABI): the value type's own, or FP64 sums of
// FP32 values -- a mixed plan.  Such a plan's sum bytes are sb = W x 8 while its value bytes stay 4: its classes, lists,
// needs and both launch plans are the FP64 plan's of the same patterns and width (every function here that takes vb
// serves that sb), and only val_static_lds, the stage of values, is asked at vb = 4.  Its backward runs the float
// kernels on that launch list: their guards at W x 4 accept whatever the guards at W x 8 accept
// (tests/valplan_mixed_check.cpp).
enum ValAccum : int { VAL_ACC_NATIVE = 0, VAL_ACC_F64 = 1 };
constexpr bool val_accum_ok(int acc) { return acc == VAL_ACC_NATIVE || acc == VAL_ACC_F64; }
__host__ __device__ constexpr int val_sum_bytes(int vb, int width, int acc) {
    return width * (acc == VAL_ACC_F64 ? VAL_VB_F64 : vb);
}

// LDS bytes of one row, per method
__host__ __device__ constexpr long long val_lds_search(long long n, int vb = VAL_VB_F64) {  // sums, then columns
    return val_search_entry(vb) * ((n + 1) & ~1LL);
}
__host__ __device__ constexpr long long val_lds_direct(long long span, int vb = VAL_VB_F64) { return vb * span; }

// The largest rows of the wave and block classes
__host__ __device__ constexpr int val_wave_direct_span(int vb) { return VAL_WAVE_BYTES / vb; }
__host__ __device__ constexpr int val_wave_search_n(int vb) { return VAL_WAVE_BYTES / val_search_entry(vb) & ~1; }
__host__ __device__ constexpr int val_block_direct_span(int vb) { return VAL_BLOCK_BYTES / vb; }
__host__ __device__ constexpr int val_block_search_n(int vb) { return VAL_BLOCK_BYTES / val_search_entry(vb) & ~1; }
constexpr int VAL_WAVE_DIRECT_SPAN = val_wave_direct_span(VAL_VB_F64);    // 1024   (FP32: 2048)
constexpr int VAL_WAVE_SEARCH_N = val_wave_search_n(VAL_VB_F64);          // 682    (FP32: 1024)
constexpr int VAL_BLOCK_DIRECT_SPAN = val_block_direct_span(VAL_VB_F64);  // 19968  (FP32: 39936)
constexpr int VAL_BLOCK_SEARCH_N = val_block_search_n(VAL_VB_F64);        // 13312  (FP32: 19968)
constexpr bool val_caps_fit(int vb) {
    return val_lds_search(VAL_TEAM_NMAX, vb) * VAL_TEAM_ROWS <= 65536 &&  // team launch below the attribute threshold
           val_lds_direct(val_wave_direct_span(vb), vb) <= VAL_WAVE_BYTES &&
           val_lds_search(val_wave_search_n(vb), vb) <= VAL_WAVE_BYTES &&
           val_lds_direct(val_block_direct_span(vb), vb) <= VAL_BLOCK_BYTES &&
           val_lds_search(val_block_search_n(vb), vb) <= VAL_BLOCK_BYTES;
}
static_assert(val_caps_fit(VAL_VB_F64) && val_caps_fit(VAL_VB_F32), "rows fit their team, wave and block slices");
// The team launch at its cap, and whether it is past what a launch may take without hipFuncSetAttribute: the team
// kernels of such an sb are registered for val_team_launch_cap (init_values_attributes)
constexpr int VAL_LDS_PLAIN = 65536;
constexpr int val_team_launch_cap(int sb) { return (int)val_lds_search(VAL_TEAM_NMAX, sb) * VAL_TEAM_ROWS; }
constexpr bool val_team_registers(int sb) { return val_team_launch_cap(sb) > VAL_LDS_PLAIN; }
constexpr bool val_caps_fit_wide(int sb) {
    return val_team_launch_cap(sb) <= LDS_MAX_C && val_lds_direct(val_wave_direct_span(sb), sb) <= VAL_WAVE_BYTES &&
           val_lds_search(val_wave_search_n(sb), sb) <= VAL_WAVE_BYTES &&
           val_lds_direct(val_block_direct_span(sb), sb) <= VAL_BLOCK_BYTES &&
           val_lds_search(val_block_search_n(sb), sb) <= VAL_BLOCK_BYTES;
}
static_assert(val_caps_fit_wide(16) && val_caps_fit_wide(32) && !val_team_registers(4) && !val_team_registers(8) &&
                  !val_team_registers(16) && val_team_registers(32) && val_team_launch_cap(32) == 73728,
              "wide rows fit their slices; the sb = 32 team launch is the registered one");
static_assert(val_wave_direct_span(16) == 512 && val_wave_search_n(16) == 408 && val_block_direct_span(16) == 9984 &&
                  val_block_search_n(16) == 7986 && val_wave_direct_span(32) == 256 && val_wave_search_n(32) == 226 &&
                  val_block_direct_span(32) == 4992 && val_block_search_n(32) == 4436,
              "the width table of the header comment");
static_assert(VAL_BLOCK_BYTES + VAL_STAGE_BYTES <= 163840, "block rows fit one workgroup");
static_assert(VAL_WAVE_DIRECT_SPAN == 1024 && VAL_WAVE_SEARCH_N == 682 && VAL_BLOCK_DIRECT_SPAN == 19968 &&
                  VAL_BLOCK_SEARCH_N == 13312 && val_wave_direct_span(4) == 2048 && val_wave_search_n(4) == 1024 &&
                  val_block_direct_span(4) == 39936 && val_block_search_n(4) == 19968,
              "the class table of the header comment");

// The guards of a row's LDS slice of `region` bytes (val_row, search_slice, the team kernels: mhs_valwalk.hpp).
// Searched: the entries the slice holds, sums first and as many columns behind them; a row of more is left alone.
__host__ __device__ constexpr int val_slice_entries(int region, int vb) { return region / val_search_entry(vb); }
// Direct: whether span-indexed sums of `span` columns fit.
__host__ __device__ constexpr bool val_slice_fits(long long span, int region, int vb) {
    return span > 0 && span <= region / vb;
}

// The class of a row: n C entries over `span` columns, `products` products (saturated); vb: the value's bytes.
__host__ __device__ inline int val_class(int n, long long span, long long products, int vb = VAL_VB_F64) {
    if (n <= 0) return VC_NONE;
    if (n <= VAL_TEAM_NMAX && products <= VAL_TEAM_PMAX) return VC_TEAM;
    if (products <= 0) return VC_GLOBAL;  // zero fill only: no LDS, nothing staged
    const bool wave = products <= VAL_WAVE_PMAX;
    if (wave && span <= val_wave_direct_span(vb)) return VC_WAVE_DIRECT;
    if (span <= val_block_direct_span(vb) && span <= (long long)VAL_DENSE_RATIO * n) return VC_BLOCK_DIRECT;
    if (wave && n <= val_wave_search_n(vb)) return VC_WAVE_SEARCH;
    if (span <= val_block_direct_span(vb)) return VC_BLOCK_DIRECT;
    if (n <= val_block_search_n(vb)) return VC_BLOCK_SEARCH;
    return VC_GLOBAL;
}
// How a masked plan may compute its rows (mhs_mask_form of the C ABI)
enum ValMaskForm : int { VM_AUTO = 0, VM_PRODUCT = 1, VM_DOT = 2 };
// smallest k with 2^k >= x (x >= 1)
__host__ __device__ inline int val_ceil_log2(long long x) {
    int k = 0;
    while (k < 62 && (1LL << k) < x) ++k;
    return k;
}
// Search steps of one mask entry against a B^T row of `len` entries: the lower bound and the look at its result
__host__ __device__ inline long long val_dot_steps(long long len) { return 1 + val_ceil_log2(len + 1); }
constexpr long long VAL_SAT = 0x7fffffffffffffffLL;
__host__ __device__ inline long long val_sat_add(long long a, long long b) { return a > VAL_SAT - b ? VAL_SAT : a + b; }
__host__ __device__ inline long long val_sat_mul(long long a, long long b) {
    return a > 0 && b > 0 && a > VAL_SAT / b ? VAL_SAT : a * b;
}
// The class of a masked plan's row: nA entries in A's row, dot_cost = nA x the sum of val_dot_steps
// over the row's mask entries (saturated).  ratio: VAL_DOT_RATIO, or the diagnostic override.
__host__ __device__ inline int val_class_masked(int n, long long span, long long products, int nA, long long dot_cost,
                                                int form, int ratio = VAL_DOT_RATIO, int vb = VAL_VB_F64) {
    const bool can = n > 0 && nA > 0;
    if (can && form == VM_DOT) return VC_DOT;
    if (can && form == VM_AUTO && val_sat_mul(ratio, dot_cost) < products) return VC_DOT;
    return val_class(n, span, products, vb);
}
// LDS bytes a row needs in its class (0: none)
__host__ __device__ inline int val_row_need(int cls, int n, long long span, int vb = VAL_VB_F64) {
    switch (cls) {
    case VC_TEAM:
    case VC_WAVE_SEARCH:
    case VC_BLOCK_SEARCH: return (int)val_lds_search(n, vb);
    case VC_WAVE_DIRECT:
    case VC_BLOCK_DIRECT: return (int)val_lds_direct(span, vb);
    default: return 0;
    }
}
// The most a row of the class can need
constexpr int val_class_cap(int cls, int vb = VAL_VB_F64) {
    return cls == VC_TEAM ? (int)val_lds_search(VAL_TEAM_NMAX, vb)
           : cls == VC_WAVE_DIRECT || cls == VC_WAVE_SEARCH ? VAL_WAVE_BYTES
           : cls == VC_BLOCK_DIRECT || cls == VC_BLOCK_SEARCH ? VAL_BLOCK_BYTES
                                                              : 0;
}

// What k_val_classify counts: rows per class and the largest row's LDS need per class.
struct ValCounts {
    int rows[VAL_NCLASS];
    int need[VAL_NCLASS];
};

// k_val_classify's counter block, as int offsets: per class the rows, the list cursor of the fill pass
// and the need, every counter on a 128-byte line of its own (BINCNT_STRIDE ints apart), then two
// 64-bit counts: the pattern's products and (masked plans: launch_val_count_kept) the kept ones.
constexpr int val_cnt_rows(int c) { return c * BINCNT_STRIDE; }
constexpr int val_cnt_cursor(int c) { return (VAL_NCLASS + c) * BINCNT_STRIDE; }
constexpr int val_cnt_need(int c) { return (2 * VAL_NCLASS + c) * BINCNT_STRIDE; }
constexpr int VAL_CNT_PRODUCTS = 3 * VAL_NCLASS * BINCNT_STRIDE;
constexpr int VAL_CNT_WIDE = BINCNT_STRIDE > 2 ? BINCNT_STRIDE : 2;  // (a 64-bit count is two ints, whatever the stride)
constexpr int VAL_CNT_KEPT = VAL_CNT_PRODUCTS + VAL_CNT_WIDE;
constexpr int VAL_CNT_INTS = VAL_CNT_KEPT + VAL_CNT_WIDE;

// Plan creation's status words: the first bad row of each check (atomicMin; none: still the fill value)
enum ValStatus : int {
    VS_APTR,      // A.ptr
    VS_BPTR,      // B.ptr
    VS_CPTR,      // C.ptr
    VS_ACOL,      // A's columns
    VS_CCOL,      // C's columns
    VS_PRODUCTS,  // a product's column missing in C
    VS_BCOL,      // B's columns (masked plans)
    VS_COUNT,
};
constexpr int VAL_STATUS_INTS = (VS_COUNT + 1) & ~1;  // whole 8-byte words

enum ValKernel : int {
    VK_TEAM,          // k_val_team
    VK_WAVE_DIRECT,   // k_val_wave<direct>
    VK_WAVE_SEARCH,   // k_val_wave<search>
    VK_BLOCK_DIRECT,  // k_val_block<T, direct>
    VK_BLOCK_SEARCH,  // k_val_block<T, search>
    VK_GLOBAL,        // k_val_global
    VK_DOT,           // k_val_dot
};

// One launch.  `region`: LDS bytes per row in flight (team slice, wave slice, or the block's all).
struct ValLaunch {
    int kernel;  // ValKernel
    int cls;     // the class whose list it walks
    int grid, block, lds;
    int region;
    int count;
};
constexpr int VAL_PLAN_MAX = 8;
struct ValPlan {
    int n;
    ValLaunch launch[VAL_PLAN_MAX];
};

// Static LDS of a forward kernel, and of its backward, at value size vb and width W, beside its launch's dynamic
// bytes: the stage of A entries of the wave and block walks (B row start and length; the A value too at W = 1 only:
// wider walks read it from A.val) and the dot class's stage (column and W values).  The kernels assert their stages
// against it.
constexpr int val_static_lds(int kernel, int vb, int width) {
    const int entry = 8 + (width == 1 ? vb : 0);
    return kernel == VK_WAVE_DIRECT || kernel == VK_WAVE_SEARCH     ? WPB * 64 * entry
           : kernel == VK_BLOCK_DIRECT || kernel == VK_BLOCK_SEARCH ? VAL_STAGE * entry
           : kernel == VK_DOT                                       ? WPB * 64 * (4 + width * vb)
                                                                    : 0;
}

constexpr int VAL_TEAM_GRID = 16384;   // block caps (rows past them are walked grid-stride)
constexpr int VAL_WAVE_GRID = 16384;
constexpr int VAL_BLOCK_GRID = 4096;
constexpr int VAL_GLOBAL_GRID = 1024;

inline int val_round(int need, int step, int cap) {
    const int b = (need + step - 1) / step * step;
    return need <= 0 || b > cap ? cap : b;
}

// The launches of a hot call, heaviest rows first (they all go on the call's stream).  c: counted at vb.
inline ValPlan plan_values(const ValCounts& c, int vb = VAL_VB_F64) {
    ValPlan p{};
    auto add = [&](int kernel, int cls, long long blocks, int cap, int threads, int lds, int region) {
        if (p.n >= VAL_PLAN_MAX) return;
        ValLaunch& l = p.launch[p.n++];
        l.kernel = kernel;
        l.cls = cls;
        l.grid = (int)(blocks < cap ? blocks : cap);
        l.block = threads;
        l.lds = lds;
        l.region = region;
        l.count = c.rows[cls];
    };
    // dot rows (masked plans only): a wave per row, static LDS only
    if (c.rows[VC_DOT] > 0) add(VK_DOT, VC_DOT, ((long long)c.rows[VC_DOT] + WPB - 1) / WPB, VAL_WAVE_GRID, 64 * WPB, 0, 0);
    if (c.rows[VC_GLOBAL] > 0) add(VK_GLOBAL, VC_GLOBAL, c.rows[VC_GLOBAL], VAL_GLOBAL_GRID, 1024, 0, 0);
    for (int k = 0; k < 2; ++k) {
        const int cls = k ? VC_BLOCK_DIRECT : VC_BLOCK_SEARCH;
        if (c.rows[cls] <= 0) continue;
        const int lds = val_round(c.need[cls], 2048, VAL_BLOCK_BYTES);
        add(k ? VK_BLOCK_DIRECT : VK_BLOCK_SEARCH, cls, c.rows[cls], VAL_BLOCK_GRID, lds <= VAL_BLOCK_SMALL ? 256 : 1024, lds, lds);
    }
    for (int k = 0; k < 2; ++k) {
        const int cls = k ? VC_WAVE_DIRECT : VC_WAVE_SEARCH;
        if (c.rows[cls] <= 0) continue;
        const int region = val_round(c.need[cls], 256, VAL_WAVE_BYTES);
        add(k ? VK_WAVE_DIRECT : VK_WAVE_SEARCH, cls, ((long long)c.rows[cls] + WPB - 1) / WPB, VAL_WAVE_GRID, 64 * WPB, WPB * region,
            region);
    }
    if (c.rows[VC_TEAM] > 0) {
        const int region = val_round(c.need[VC_TEAM], 2 * val_search_entry(vb), val_class_cap(VC_TEAM, vb));
        add(VK_TEAM, VC_TEAM, ((long long)c.rows[VC_TEAM] + VAL_TEAM_ROWS - 1) / VAL_TEAM_ROWS, VAL_TEAM_GRID, 256,
            VAL_TEAM_ROWS * region, region);
    }
    return p;
}

// The launches of a backward call (mhs_spgemm_values_grad, mhs_spgemm_values_grad_batched; vb: the plan's sum
// bytes): the forward's, each run by its class's backward
// kernel (mhs_values_grad.hip), but for the dot rows of a masked plan -- there is no dot-form backward: their
// list goes to the global-form kernel, a wave per row (block 256; the global class runs it 1024 threads a row).
inline ValPlan plan_grad(const ValCounts& c, int vb = VAL_VB_F64) {
    ValPlan p = plan_values(c, vb);
    for (int i = 0; i < p.n; ++i)
        if (p.launch[i].kernel == VK_DOT) p.launch[i].kernel = VK_GLOBAL;  // (cls stays VC_DOT: the list it walks)
    return p;
}

}  // namespace mhs
