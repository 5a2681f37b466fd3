// mhs_api.cpp -- C-ABI orchestration of the MI355X SpGEMM (include/mhspgemm.h).
//
// Replaces MH_spgemm (reference src/main.cu:12-72) and the Tool workspace
// (src/Tool.cu:4-69).  One call = one stream-ordered pipeline:
//
//   memset stats -> k_mask_b (Form_mask_matrix_B) -> k_analyze + bins (symbolic_binning)
//   -> symbolic bins (Calculate_C_nnz) -> scan + classify + bins + ONE readback
//   (numeric_binning) -> C.col/C.val allocation (Malloc_C_col_val) -> numeric bins
//   (Numeric) -> stream sync.
//
// The reference makes 5 binning round trips (2 blocking copies each), 3 scalar
// reads and 6 device-wide syncs per call; here the only host round
// trip is the single Stats readback that C's allocation needs anyway.
//
// On the host, mhs_spgemm checks its arguments and runs spgemm_attempt (again after a
// speculation miss); an attempt is one Call taken through its phases
//   plan_workspace -> analyze_rows -> choose_plan -> launch_symbolic -> launch_scan
//   -> speculate_numeric (phase A of the previous call's plan) -> handoff
//   -> finish_speculated (phase B, or the miss) -> numeric_after_handoff -> finish_call
// and C's arrays belong to the Call's owner (mhs_owner.hpp) until finish_call commits.
// Around the call, the context's own entry points: creation and options, streams, the output pool
// (mhs_ctx_recycle, mhs_ctx_trim), mhs_transpose, the diagnostics.  The context itself (mhs_ctx) and the
// entry points' error helpers are in mhs_ctx.hpp; the values plans and their calls in mhs_values_api.cpp.
#include "mhs_ctx.hpp"
#include "mhs_owner.hpp"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

using namespace mhs;

namespace {

// Spin until the device has published call `seq`'s Stats.  Every 256 polls the
// stream is queried: a fault ends the wait with the HIP error, an idle stream
// without the publication is an internal error (never spins forever).
int wait_published(mhs_ctx* ctx, hipStream_t s, const Published* pub, int seq) {
    for (unsigned polls = 1;; ++polls) {
        if (__atomic_load_n(&pub->seq, __ATOMIC_ACQUIRE) == seq) return MHS_OK;
        if ((polls & 255) == 0) {
            const hipError_t q = hipStreamQuery(s);
            if (q == hipSuccess) {
                if (__atomic_load_n(&pub->seq, __ATOMIC_ACQUIRE) == seq) return MHS_OK;
                return fail(ctx, MHS_ERR_HIP, "device did not publish the symbolic statistics");
            }
            if (q != hipErrorNotReady) return fail_hip(ctx, q, "waiting for the symbolic phase");
        }
#if defined(__x86_64__)
        __builtin_ia32_pause();
#endif
    }
}

double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

hipError_t pool_get(mhs_ctx* ctx, void** p, size_t bytes) {
    if (bytes == 0) bytes = 16;
    size_t best = (size_t)-1;
    size_t bi = 0;
    for (size_t i = 0; i < ctx->pool.size(); ++i) {
        const size_t s = ctx->pool[i].second;
        if (s >= bytes && s <= 2 * bytes + (1u << 20) && s < best) {
            best = s;
            bi = i;
        }
    }
    if (best != (size_t)-1) {
        *p = ctx->pool[bi].first;
        ctx->pool.erase(ctx->pool.begin() + (long)bi);
        return poison_fill(ctx, *p, best, ctx->stream);  // (MHS_POISON: not what its last owner left in it)
    }
    hipError_t e = hipMalloc(p, bytes);
    if (e == hipErrorOutOfMemory && !ctx->pool.empty()) {
        for (auto& b : ctx->pool) (void)hipFree(b.first);
        ctx->pool.clear();
        (void)hipGetLastError();
        e = hipMalloc(p, bytes);
    }
    if (e == hipSuccess) e = poison_fill(ctx, *p, bytes, ctx->stream);
    return e;
}

// The buffer's true size comes from the runtime (not from a side table: a buffer
// freed with mhs_csr_free and handed out again by hipMalloc at the same address
// would otherwise be filed under its old size).
void pool_put(mhs_ctx* ctx, void* p) {
    if (!p) return;
    hipDeviceptr_t base = nullptr;
    size_t bytes = 0;
    if (hipMemGetAddressRange(&base, &bytes, (hipDeviceptr_t)p) != hipSuccess || base != (hipDeviceptr_t)p) {
        (void)hipGetLastError();
        (void)hipFree(p);
        return;
    }
    ctx->pool.emplace_back(p, bytes);
    // keep the pool bounded: drop the oldest buffers beyond 16 entries
    while (ctx->pool.size() > 16) {
        (void)hipFree(ctx->pool.front().first);
        ctx->pool.erase(ctx->pool.begin());
    }
}

// The owner of a call's C arrays (mhs_owner.hpp): released into the pool or freed, after a
// wait for the call's stream and the aux streams a call forks to.
struct OwnerOps {
    static void release(mhs_ctx* ctx, void* p, bool pooled) {
        if (pooled) pool_put(ctx, p);
        else if (p) (void)hipFree(p);
    }
    static void sync(mhs_ctx* ctx) {
        (void)hipStreamSynchronize(ctx->stream);
        for (hipStream_t x : ctx->aux)
            if (x) (void)hipStreamSynchronize(x);
        (void)hipGetLastError();
    }
};
using Owner = OutputOwner<mhs_ctx, OwnerOps>;

struct Layout {
    size_t btcol, btmask, bmeta, bhi, rflop, rtflop, rlo, rhi, ctiles, sym_bin, asame, grp, bin_list, scan_part, mcache,
        stats, blkflop, spill_mask, spill_key, lofs, tslot, nft_bin, near_list, nsig, ucol, gna, bx_col, bx_val, split_list, total;
    bool near, near_b;
    long long bx_pre;  // B's entries in front of the union rows in bx_* (B is A), else 0
    long long spill_cap;
};

// near: near row groups planned; near_b: B is A (the union rows also serve B's union runs, so
// B's arrays are copied in front of them -- A != B reserves only the union rows)
Layout plan(int M, int MB, long long nnzA, long long nnzB, int mc_list, int M_total = -1, bool near = false,
            bool near_b = false) {
    Layout L{};
    size_t o = 0;
    auto take = [&](size_t bytes) {
        size_t r = o;
        o += al(bytes ? bytes : 16);
        return r;
    };
    const size_t nscan = (size_t)(M + 1 + SCAN_ITEMS - 1) / SCAN_ITEMS + 1;
    L.stats = take(sizeof(Stats));
    L.btcol = take((size_t)nnzB * 4);
    L.btmask = take((size_t)nnzB * 8);
    L.bmeta = take((size_t)MB * 16);
    L.bhi = take((size_t)MB * 4);
    L.rflop = take((size_t)M * 4);
    L.rtflop = take((size_t)M * 4);
    L.rlo = take((size_t)M * 4);
    L.rhi = take((size_t)M * 4);
    L.ctiles = take((size_t)M * 4);
    L.sym_bin = take((size_t)M);
    L.asame = take((size_t)M);
    L.grp = take((size_t)M);
    static_assert((int)NUM_NB >= (int)SYM_NB, "bin_list holds either phase's bins");
    L.bin_list = take((size_t)(NUM_NB - 1) * M * 4);
    L.blkflop = take(((size_t)analyze_launch(nnzA, M).words + 1) * 8);
    L.scan_part = take(nscan * 8 + (size_t)ZERO_INTS * 4);  // look-back words, then the row cursors and bin counters
    L.mcache = take((size_t)M * mc_stride(mc_list) * 8);
    L.spill_cap = spill_cap(nnzB);
    if (M_total > M && M_total > 0)  // a row chunk: its share of the region (spill lists belong to rows)
        L.spill_cap = std::max<long long>(SPILL_PARTS * 1024, L.spill_cap * M / M_total);
    if (const char* e = getenv("MHS_SPILL_CAP")) L.spill_cap = atoll(e) < 1 ? 1 : atoll(e);  // tests: a full region
    L.spill_mask = take((size_t)L.spill_cap * 8);
    L.spill_key = take((size_t)L.spill_cap * 4);
    L.lofs = take((size_t)M * 4);
    L.tslot = take((size_t)M * 8);
    L.nft_bin = take((size_t)M);
    L.split_list = take((size_t)M * 4);
    L.near = near;
    if (near) {  // near row groups: candidate list, union rows (see Work)
        L.near_b = near_b;
        L.bx_pre = near_b ? nnzB : 0;
        L.near_list = take((size_t)M * 4);
        L.nsig = take((size_t)M * 4);
        L.ucol = take((size_t)nnzA * 4);
        L.gna = take((size_t)M * 4);
        if (near_b) L.bx_col = take((size_t)(nnzB + 3 * nnzA) * 4);  // B's arrays + the union rows (see Work)
        L.bx_val = take((size_t)(L.bx_pre + 3 * nnzA) * 8);
    }
    L.total = o;
    return L;
}

// Device bytes the context holds for a call: its cached buffers plus C arrays a row-chunked
// call has already allocated (MHS_OPT_MEM_BUDGET counts them all).
size_t held(const mhs_ctx* ctx) { return ctx->ws_bytes + ctx->gscratch_bytes + ctx->slots_bytes + ctx->c_held; }

int ensure(mhs_ctx* ctx, char** buf, size_t* have, size_t need) {
    if (*have >= need) return MHS_OK;
    if (*buf) {
        MHS_HIP(hipStreamSynchronize(ctx->stream));
        MHS_HIP(hipFree(*buf));
        *buf = nullptr;
        *have = 0;
    }
    size_t want = need + need / 8;
    if (ctx->mem_budget && held(ctx) + want > ctx->mem_budget) want = need;
    if (ctx->mem_budget && held(ctx) + need > ctx->mem_budget)
        return fail(ctx, MHS_ERR_OOM, "workspace exceeds the context's memory budget");
    MHS_HIP(hipMalloc((void**)buf, want));
    *have = want;
    MHS_HIP(poison_fill(ctx, *buf, want, ctx->stream));
    return MHS_OK;
}

// C.col / C.val of nnz entries (+ what the call already holds) within the test budget
hipError_t alloc_c(mhs_ctx* ctx, mhs_csr* out, long long nnz) {
    if (ctx->mem_budget && held(ctx) + (size_t)nnz * 12 > ctx->mem_budget) return hipErrorOutOfMemory;
    hipError_t e = pool_get(ctx, (void**)&out->col, (size_t)nnz * 4);
    if (e == hipSuccess) e = pool_get(ctx, (void**)&out->val, (size_t)nnz * 8);
    if (e != hipSuccess) {
        pool_put(ctx, out->col);
        out->col = nullptr;
    }
    return e;
}

// The call's Work over the workspace laid out by `L` (rows of this pass: M).
Work make_work(mhs_ctx* ctx, const Layout& L, int M, long long nnzA, long long nnzB, int mc_list) {
    Work w{};
    w.btcol = (int*)(ctx->ws + L.btcol);
    w.btmask = (unsigned long long*)(ctx->ws + L.btmask);
    w.bmeta = (int4*)(ctx->ws + L.bmeta);
    w.bhi = (int*)(ctx->ws + L.bhi);
    w.rflop = (int*)(ctx->ws + L.rflop);
    w.rtflop = (int*)(ctx->ws + L.rtflop);
    w.rlo = (int*)(ctx->ws + L.rlo);
    w.rhi = (int*)(ctx->ws + L.rhi);
    w.ctiles = (int*)(ctx->ws + L.ctiles);
    w.sym_bin = (unsigned char*)(ctx->ws + L.sym_bin);
    w.asame = (unsigned char*)(ctx->ws + L.asame);
    w.grp = (unsigned char*)(ctx->ws + L.grp);
    w.groups = ctx->groups ? 1 : 0;
    w.tiny_num = ctx->tiny_num ? 1 : 0;  // per row: packed sort keys hold its column offsets in 23 bits
    w.bin_list = (int*)(ctx->ws + L.bin_list);
    w.blkflop = (unsigned long long*)(ctx->ws + L.blkflop);
    w.nflop = analyze_launch(nnzA, M).words;
    w.scan_part = (int*)(ctx->ws + L.scan_part);
    w.cursors = w.scan_part + 2 * ((M + 1 + SCAN_ITEMS - 1) / SCAN_ITEMS + 1);
    w.mcache = ctx->use_mcache ? (unsigned long long*)(ctx->ws + L.mcache) : nullptr;
    w.mc_list = mc_list;
    w.spill.mask = (unsigned long long*)(ctx->ws + L.spill_mask);
    w.spill.key = (int*)(ctx->ws + L.spill_key);
    w.spill.lofs = (int*)(ctx->ws + L.lofs);
    w.spill.top = w.cursors + SPILL_CURSOR_SLOT * 8 * CURSOR_STRIDE;  // zeroed with the cursors
    w.spill.cap = L.spill_cap;
    w.tslot = (long long*)(ctx->ws + L.tslot);
    w.split_list = (int*)(ctx->ws + L.split_list);
    if (L.near) {
        w.near_list = (int*)(ctx->ws + L.near_list);
        w.nsig = (unsigned*)(ctx->ws + L.nsig);
        w.ucol = (int*)(ctx->ws + L.ucol);
        w.bx_val = (double*)(ctx->ws + L.bx_val);
        w.uval = w.bx_val + L.bx_pre;
        if (L.near_b) {  // B is A: its union runs read bx_*
            w.bx_col = (int*)(ctx->ws + L.bx_col);
            w.ucolx = w.bx_col + nnzB;
        }
        w.gna = (int*)(ctx->ws + L.gna);
    }
    w.stats = (Stats*)(ctx->ws + L.stats);
    w.gscratch = ctx->gscratch;
    w.gscratch_bytes = ctx->gscratch_bytes;
    return w;
}

std::string err_text(int err) {
    std::string m;
    if (err & ERR_UNSORTED) m += "B column indices are not sorted within a row; ";
    if (err & ERR_COL_RANGE) m += "B column index out of [0, B.N); ";
    if (err & ERR_ACOL_RANGE) m += "A column index out of [0, B.M); ";
    if (err & ERR_OVERFLOW) m += "nnz(C) exceeds INT32_MAX; ";
    return m;
}

// The device-side checks' verdict (Stats::err != 0) as the call's error.
int fail_stats(mhs_ctx* ctx, int err) {
    return fail(ctx, (err & ERR_OVERFLOW) ? MHS_ERR_OVERFLOW : MHS_ERR_INVALID, err_text(err));
}

// mhs_timing's bin counters from per-bin row counts ([0]: the rows in no bin).
void fill_bins(mhs_timing& tm, int M, const int* sym, const int* num) {
    static_assert(NBINS <= sizeof tm.sym_bins / sizeof tm.sym_bins[0], "mhs_timing holds every bin");
    long long ns = 0, nn = 0;
    for (int i = 1; i < NBINS; ++i) {
        ns += tm.sym_bins[i] = sym[i];
        nn += tm.num_bins[i] = num[i];
    }
    tm.sym_bins[0] = (int)(M - ns);
    tm.num_bins[0] = (int)(M - nn);
}

// Everything before the numeric launches for the rows of `a` (M > 0): (mask of B), row
// analysis, symbolic bins, row_ptr scan into Cptr[0..M] + numeric bins, the Stats hand-off.
// The plans of a pass without the probe, near groups, a fork or a speculated plan, on one stream.
int front_pass(mhs_ctx* ctx, const Csr& a, const Csr& b, Work& w, int* Cptr, bool mask, Stats& h) {
    hipStream_t s = ctx->stream;
    if (!ctx->stats_zero) MHS_HIP(hipMemsetAsync(w.stats, 0, sizeof(Stats), s));
    ctx->stats_zero = false;
    const FrontShape sh{a.M, b.M, a.nnz, b.nnz, mask};
    const FrontPointers fp{a, b, w, Cptr, ctx->dense_span_max, ctx->d_pub};
    for (const FrontPlan& p : {plan_front_rows(sh), plan_front_symbolic(sh, nullptr)})
        for (int i = 0; i < p.n; ++i) issue_front(p.launch[i], fp, s);
    const int seq = ++ctx->seq;
    issue_front(front_scan(a.M), fp, s, seq);
    MHS_HIP(hipGetLastError());
    const int rc = wait_published(ctx, s, ctx->pub, seq);
    if (rc) return rc;
    memcpy(&h, (const void*)&ctx->pub->stats, sizeof(Stats));
    ctx->stats_zero = true;
    ++ctx->front_passes;
    return MHS_OK;
}

constexpr int NUM_GLOBAL_GRID = 128;
#ifndef MHS_MULTI_FLOP_LOG2
#define MHS_MULTI_FLOP_LOG2 22  // numeric launches over several streams from 2^this products on (round 4: 24 -> 22, scircuit-like numeric -9 %)
#endif

#ifndef MHS_SPLIT_FLOP_LOG2
#define MHS_SPLIT_FLOP_LOG2 24  // block bins split by LDS need from 2^this products on
#endif

// Streams the numeric launches of `h` are dealt over: several heavy bins go over the aux
// streams (fork/join costs ~10-20 us, so only for at least 3 launches of a product worth it).
int numeric_streams(const mhs_ctx* ctx, const Stats& h) {
    const int nl = numeric_launches(h);
    return (nl >= 3 && h.flop >= (1ull << MHS_MULTI_FLOP_LOG2)) ? std::min(ctx->num_streams, nl) : 1;
}

// The numeric launches for `h` (grids, LDS) on the call's stream, the heavy bins dealt over
// the aux streams, which join the call's stream again.
// Phases of a numeric launch sequence: ALL (after the hand-off: every launch), and the two halves
// of a speculated plan -- SPEC_A, queued right behind k_scan before its Stats are known: the fork
// event, the block-bin split and the launches dealt to the call's stream; SPEC_B, after the host
// has seen k_scan's verdict: the aux streams' launches (their wait on the fork event then finds
// it complete -- waits on a pending one measured slower than the whole hand-off, r06b) and joins.
enum NumPhase { NUM_ALL = 0, NUM_SPEC_A = 1, NUM_SPEC_B = 2 };

NumShape num_shape(const mhs_ctx* ctx, const Csr& a, const Csr& b, const Work& w, bool split) {
    return NumShape{a.M, a.nnz, b.nnz, w.bx_on, w.sc_col != nullptr, split, NUM_GLOBAL_GRID, ctx->cus, ctx->group_cap,
                    ctx->no_o32};
}

// `plan`: built by the phase that runs first (ALL, SPEC_A) and kept by the caller for SPEC_B.
int run_numeric(mhs_ctx* ctx, const Csr& a, const Csr& b, const Work& w, const Stats& h, const mhs_csr& out,
                NumPlan& plan, hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr, int phase = NUM_ALL) {
    hipStream_t s = ctx->stream;
    // several heavy bins: deal them over the aux streams (fork/join costs ~10-20 us,
    // so only when there are at least 3 launches of a product worth it)
    hipStream_t ss[mhs_ctx::NAUX + 1] = {s};
    int nss = numeric_streams(ctx, h);
    if (w.go) nss = std::min(nss, ctx->spec_nss);  // (MHS_SPEC_NSS: a speculated plan on fewer streams)
    for (int i = 1; i < nss; ++i) ss[i] = ctx->aux[i - 1];
    const bool first = phase != NUM_SPEC_B, last = phase != NUM_SPEC_A;
    if (phase == NUM_SPEC_B && nss == 1) return MHS_OK;  // (phase A launched everything)
    if (first && nss > 1 && ev0) MHS_HIP(hipEventRecord(ev0, s));  // (several streams: events of their own)
    if (first && nss > 1) MHS_HIP(hipEventRecord(ctx->fork_ev, s));
    // block bins split by LDS need only where their two launches can run side by side (on
    // one stream the hub rows' launch would no longer overlap the others' bulk).  The partition
    // runs on the call's stream after the fork: only the split launches wait for it (split_ev),
    // the other bins start at once (wb-edu-like: 0.33 ms off the numeric phase's start)
    // (and only from 2^MHS_SPLIT_FLOP_LOG2 products: on scircuit-like the partition and its event
    // wait cost more than the split saves -- numeric 0.146 -> 0.119 ms unsplit)
    if (first) {
        const bool want_split = nss > 1 && ctx->split && h.flop >= (1ull << MHS_SPLIT_FLOP_LOG2);
        const bool split = want_split && launch_split_bins(w, h, a.M, out.ptr, s, ctx->dense_span_max);
        if (split) MHS_HIP(hipEventRecord(ctx->split_ev, s));
        ctx->stat[MHS_STAT_SPLIT] += split;
        ctx->stat[MHS_STAT_MULTI_STREAM] += nss > 1;
        plan = plan_numeric(h, num_shape(ctx, a, b, w, split));
    }
    // Launch i on ss[stream_of(i, nss)]; a speculated plan's phase A issues the call stream's share,
    // phase B the rest.  The aux streams wait for the fork event (everything before numeric): waits
    // set up once, right before the first launch that lands on an aux stream -- after launch 0 has
    // gone out on the call's stream (host API calls that would otherwise sit between the hand-off and
    // the first numeric kernel: round 5, scircuit-like's hand-off gap).  A failed wait sends every
    // later launch to ss[0]: no aux-stream launch may run without its dependency on the pre-numeric
    // work.  On one stream the timing events ride on the first and the last dispatch.
    const NumPointers np{a, b, w, out.ptr, out.col, out.val, ctx->dense_span_max};
    hipError_t fe = hipSuccess;
    bool forked = false;
    int used = 0;  // streams launched on (bit k: ss[k])
    auto fork = [&]() {
        forked = true;
        for (int i = 1; i < nss && fe == hipSuccess; ++i) fe = hipStreamWaitEvent(ss[i], ctx->fork_ev, 0);
    };
    for (int i = 0; i < plan.n; ++i) {
        const NumLaunch& l = plan.launch[i];
        const int dealt = stream_of(i, nss);
        if (phase == NUM_SPEC_A ? dealt != 0 : phase == NUM_SPEC_B && dealt == 0) continue;
        if (dealt != 0 && !forked) fork();
        const int k = fe == hipSuccess ? dealt : 0;
        used |= 1 << k;
        if (l.after_split && k != 0) (void)hipStreamWaitEvent(ss[k], ctx->split_ev, 0);  // (k_split_bins' lists)
        issue_numeric(l, plan.o32, np, ss[k], nss == 1 && i == 0 ? ev0 : nullptr,
                      nss == 1 && i + 1 == plan.n ? ev1 : nullptr);
    }
    if (nss == 1 && plan.n == 0) {  // (no launch to carry them)
        if (ev0) MHS_HIP(hipEventRecord(ev0, s));
        if (ev1) MHS_HIP(hipEventRecord(ev1, s));
    }
    if (!forked && nss > 1 && last) fork();  // (nothing dealt to an aux stream: the error check below expects the waits)
    if (!last) {
        MHS_HIP(hipGetLastError());
        return MHS_OK;
    }
    // joins first: an error below must not leave aux-stream work behind the call's stream
    for (int i = 1; i < nss; ++i)
        if (used & (1 << i)) {
            MHS_HIP(hipEventRecord(ctx->join_ev[i - 1], ss[i]));
            MHS_HIP(hipStreamWaitEvent(s, ctx->join_ev[i - 1], 0));
        }
    if (nss > 1 && ev1) MHS_HIP(hipEventRecord(ev1, s));
    MHS_HIP(fe);
    MHS_HIP(hipGetLastError());
    return MHS_OK;
}

// Global-bin scratch for the numeric pass of `h` (grown on demand).
int ensure_gscratch(mhs_ctx* ctx, Work& w, const Stats& h) {
    if (h.num_count[NUM_GLOBAL] <= 0) return MHS_OK;
    const size_t per = (size_t)align16(h.num_global_need);
    const size_t g = (size_t)std::min(h.num_count[NUM_GLOBAL], NUM_GLOBAL_GRID);
    const int rc = ensure(ctx, &ctx->gscratch, &ctx->gscratch_bytes, per * g);
    if (rc) return rc;
    w.gscratch = ctx->gscratch;
    w.gscratch_bytes = ctx->gscratch_bytes;
    return MHS_OK;
}

void free_cached(mhs_ctx* ctx) {
    if (ctx->ws) (void)hipFree(ctx->ws);
    if (ctx->gscratch) (void)hipFree(ctx->gscratch);
    if (ctx->slots) (void)hipFree(ctx->slots);
    ctx->ws = ctx->gscratch = ctx->slots = nullptr;
    ctx->ws_bytes = ctx->gscratch_bytes = ctx->slots_bytes = 0;
    for (auto& b : ctx->pool) (void)hipFree(b.first);
    ctx->pool.clear();
    ctx->stats_zero = false;
}

// Row-chunked product, the fallback when the workspace (or the workspace and C together)
// does not fit the device.  Everything cached is given back; a counting pass runs with the
// largest chunk workspace that fits (Mc rows, halved until it does) and sizes C; the
// workspace is freed and C allocated -- C's size does not depend on the chunking, so when C
// alone does not fit the call fails right there, after one pass; then the workspace is laid
// out again for the memory C leaves (halved only while the workspace itself does not fit)
// and a second pass writes every chunk's rows at their offset in C (row_ptr rebased by one
// small kernel per chunk).  The reference has no such path: Tool::allocate and the C
// cudaMalloc simply throw (src/Tool.cu:4-45, src/main.cu:54-61).
int spgemm_chunked(mhs_ctx* ctx, const mhs_csr* A, const mhs_csr* B, mhs_csr* C, mhs_timing* t,
                   std::chrono::steady_clock::time_point T0) {
    const int M = A->M, MB = B->M;
    hipStream_t s = ctx->stream;
    MHS_HIP(hipStreamSynchronize(s));
    free_cached(ctx);
    (void)hipGetLastError();
    int Mc = M, mc_list = 0;
    Layout L{};
    const Csr b{B->M, B->N, B->nnz, B->ptr, B->col, B->val};
    auto view = [&](int c) {
        const int r0 = c * Mc, r1 = std::min(M, r0 + Mc);
        // nnz of a view only steers launch geometry: the same estimate in plan and launch
        const int est = (int)((long long)A->nnz * (r1 - r0) / (M > 0 ? M : 1));
        return Csr{r1 - r0, A->N, est, A->ptr + r0, A->col, A->val};
    };
    // the workspace for chunks of Mc rows: `first` rows, then halved until it fits (a one-row
    // workspace is tried before the call gives up)
    auto fit_workspace = [&](int first) {
        for (Mc = first;; Mc = (Mc + 1) / 2) {
            if (ctx->ws) (void)hipFree(ctx->ws);
            ctx->ws = nullptr;
            ctx->ws_bytes = 0;
            ctx->stats_zero = false;
            mc_list = ctx->mc_list > 0 ? ctx->mc_list : mc_list_for(Mc);
            L = plan(Mc, MB, A->nnz, B->nnz, mc_list, M);
            const int rc = ensure(ctx, &ctx->ws, &ctx->ws_bytes, L.total);
            if (rc != MHS_ERR_OOM) return rc;
            (void)hipGetLastError();
            if (Mc <= 1) return fail(ctx, MHS_ERR_OOM, "a one-row workspace does not fit the device");
        }
    };
    int rc = fit_workspace((M + 1) / 2);  // (the whole-M workspace has just failed)
    if (rc) return rc;
    // pass 1: counts
    int nch = (M + Mc - 1) / Mc;
    Stats h{};
    long long total = 0;
    unsigned long long flop = 0;
    {
        Owner tmp(ctx, true);  // a chunk's row_ptr
        MHS_HIP(pool_get(ctx, (void**)&tmp.out.ptr, (size_t)(Mc + 1) * 4));
        tmp.queued = true;
        for (int c = 0; c < nch && rc == MHS_OK; ++c) {
            const Csr a = view(c);
            Work w = make_work(ctx, L, a.M, a.nnz, B->nnz, mc_list);
            rc = front_pass(ctx, a, b, w, tmp.out.ptr, c == 0, h);
            if (rc == MHS_OK && h.err) rc = fail_stats(ctx, h.err);
            total += h.nnzC;
            flop += h.flop;
        }
        if (rc) return rc;
        tmp.give_back();  // (every pass has been waited for)
    }
    if (total > INT_MAX) return fail(ctx, MHS_ERR_OVERFLOW, "nnz(C) exceeds INT32_MAX (the total over the row chunks)");
    // C before the second pass's workspace: it does not depend on the chunking
    const int Mc1 = Mc;
    free_cached(ctx);
    Owner own(ctx, false);  // (a real free: the pool goes with every cached buffer here)
    mhs_csr& out = own.out;
    out.M = M;
    out.N = B->N;
    out.nnz = (int)total;
    {
        hipError_t e = pool_get(ctx, (void**)&out.ptr, (size_t)(M + 1) * 4);
        if (e == hipSuccess) e = alloc_c(ctx, &out, total);
        if (e != hipSuccess) {
            free_cached(ctx);
            (void)hipGetLastError();
            return e == hipErrorOutOfMemory ? fail(ctx, MHS_ERR_OOM, "C itself does not fit the device")
                                            : fail_hip(ctx, e, "allocating C (row-chunked)");
        }
    }
    ctx->c_held = (size_t)(M + 1) * 4 + (size_t)total * 12;
    rc = fit_workspace(Mc1);  // (pass 1 fitted Mc1 rows alone; C now sits beside it)
    ctx->c_held = 0;
    if (rc) return rc;
    nch = (M + Mc - 1) / Mc;
    // pass 2: every chunk's rows at their offset
    long long off = 0;
    int sym[NBINS] = {}, num[NBINS] = {};
    bool wide = false;  // a chunk's plan took the 64-bit offsets
    own.queued = true;
    for (int c = 0; c < nch; ++c) {
        const Csr a = view(c);
        const int r0 = c * Mc;
        Work w = make_work(ctx, L, a.M, a.nnz, B->nnz, mc_list);
        rc = front_pass(ctx, a, b, w, out.ptr + r0, c == 0, h);
        if (rc == MHS_OK) rc = ensure_gscratch(ctx, w, h);
        if (rc) return rc;
        if (h.nnzC > 0) {
            const NumPlan p = plan_numeric(h, num_shape(ctx, a, b, w, false));
            const NumPointers np{a, b, w, out.ptr + r0, out.col + off, out.val + off, ctx->dense_span_max};
            for (int i = 0; i < p.n; ++i) issue_numeric(p.launch[i], p.o32, np, s, nullptr, nullptr);
            wide |= !p.o32;
        }
        launch_add_offset(out.ptr + r0, a.M + (c == nch - 1 ? 1 : 0), (int)off, s);
        MHS_HIP(hipGetLastError());
        off += h.nnzC;
        for (int i = 1; i < NBINS; ++i) {
            sym[i] += h.sym_count[i];
            num[i] += h.num_count[i];
        }
    }
    MHS_HIP(hipStreamSynchronize(s));
    own.commit(C);
    ++ctx->chunked_calls;
    ctx->stat[MHS_STAT_WIDE_OFFSETS] += wide;
    if (t) {
        mhs_timing tm{};
        tm.total_e2e = tm.total_ref = ms_since(T0);
        tm.flop = flop;
        tm.nnzC = total;
        fill_bins(tm, M, sym, num);
        *t = tm;
    }
    return MHS_OK;
}

// Phase results beside the MHS_* codes: the row-chunked path has completed the call; the call
// runs again without speculation.
enum : int { CALL_DONE = -1, CALL_RERUN = -2 };

// One attempt at C = A * B: the state its phases hand on to each other, in the order they run.
struct Call {
    mhs_ctx* const ctx;
    const mhs_csr *const A, *const B;
    mhs_csr* const C;
    mhs_timing* const t;  // (null: no per-phase events)
    const bool rerun;     // the second attempt of a user call, after a speculation miss: not counted again
    const hipStream_t s;
    const std::chrono::steady_clock::time_point T0 = std::chrono::steady_clock::now();
    const Csr a, b;
    const int M;
    int mc_list = 0;
    Layout L{};
    Work w{};
    // numeric-first tiny rows: decided by a hand-off of k_analyze's counts (big M), or without one
    bool probe = false, nft_auto = false;
    unsigned long long other = 0;  // the probe's count of rows past the tiny classes
    bool fork_sym = false;   // the rare symbolic bins run on an aux stream
    bool plannable = false;  // this call's Stats may serve the next call as its plan
    bool spec = false;       // the previous call's plan is queued ahead of this call's Stats
    mhs_ctx::PlanKey key{};
    Stats ph{};  // the plan (a copy: this call replaces the context's)
    Stats h{};   // this call's own Stats, after the hand-off
    FrontPlan fplan{};  // the launches up to the bin lists, then (launch_symbolic) the symbolic ones
    NumPlan nplan{};  // the numeric launches (a speculated call: built by phase A, finished by phase B)
    int seq = 0;            // k_scan's publication
    bool launched = false;  // the plan's phase A went out
    SpecOutcome outcome = SPEC_PROCEED;  // spec_outcome (mhs_shape.hpp), set by finish_speculated
    hipEvent_t nev0 = nullptr, nev1 = nullptr;  // this call's slot of the numeric event ring
    double t_alloc = 0, t_malloc = 0;
    hipError_t alloc_err = hipSuccess;  // alloc_c's, from prepare_numeric
    Owner own;

    Call(mhs_ctx* x, const mhs_csr* A_, const mhs_csr* B_, mhs_csr* C_, mhs_timing* t_, bool rerun_)
        : ctx(x), A(A_), B(B_), C(C_), t(t_), rerun(rerun_), s(x->stream),
          a{A_->M, A_->N, A_->nnz, A_->ptr, A_->col, A_->val},
          b{B_->M, B_->N, B_->nnz, B_->ptr, B_->col, B_->val}, M(A_->M), own(x, true) {
        own.out.M = M;
        own.out.N = b.N;
        if (const int nring = (int)ctx->nev.size() / 2) {
            nev0 = ctx->nev[2 * (ctx->ncalls % nring)];
            nev1 = ctx->nev[2 * (ctx->ncalls % nring) + 1];
        }
    }
    // the phases, in the order spgemm_attempt runs them
    int plan_workspace();
    int analyze_rows();
    void choose_plan();
    int launch_symbolic();
    int launch_scan();
    int speculate_numeric();
    int handoff();
    int finish_speculated();
    int numeric_after_handoff();
    int finish_call();
    // their helpers
    int go_chunked();
    int prepare_numeric(const Stats& of, bool* no_room);
    int run_or_stamp(const Stats& of, int phase);
    int fill_timing(mhs_timing& tm);
    FrontShape front_shape() const { return {M, b.M, a.nnz, b.nnz, 1, probe, w.nft, w.sym_big, L.near, fork_sym}; }
    // one pre-numeric launch on the stream it names; fplan's from *i on, up to and including family `last`
    void issue(const FrontLaunch& l, int seq_ = 0, const SpecArgs* sa = nullptr) {
        issue_front(l, {a, b, w, own.out.ptr, ctx->dense_span_max, ctx->d_pub}, l.stream == FRONT_AUX ? ctx->aux[0] : s,
                    seq_, sa);
    }
    void issue_upto(int* i, int last, int seq_ = 0) {
        for (; *i < fplan.n && fplan.launch[*i].kernel <= last; ++*i) issue(fplan.launch[*i], seq_);
    }
};

int check_args(mhs_ctx* ctx, const mhs_csr* A, const mhs_csr* B, const mhs_csr* C) {
    if (!ctx) return MHS_ERR_INVALID;
    if (!A || !B || !C) return fail(ctx, MHS_ERR_INVALID, "null argument");
    if (A->M < 0 || A->N < 0 || A->nnz < 0 || B->M < 0 || B->N < 0 || B->nnz < 0)
        return fail(ctx, MHS_ERR_INVALID, "negative dimension");
    if (A->N != B->M)
        return fail(ctx, MHS_ERR_INVALID, "A.N != B.M (C = A*B needs matching inner dimension)");
    if ((A->M > 0 && !A->ptr) || (B->M > 0 && !B->ptr) || (A->nnz > 0 && (!A->col || !A->val)) ||
        (B->nnz > 0 && (!B->col || !B->val)))
        return fail(ctx, MHS_ERR_INVALID, "null device array");
    return MHS_OK;
}

// The call goes on row-chunked (its own C arrays, if any, have been handed back).
int Call::go_chunked() {
    const int rc = spgemm_chunked(ctx, A, B, C, t, T0);
    return rc == MHS_OK ? CALL_DONE : rc;
}

// ---- mem_alloc: workspace (cached across calls) + C.ptr; zeroed device Stats
int Call::plan_workspace() {
    mc_list = ctx->mc_list > 0 ? ctx->mc_list : mc_list_for(M);
    probe = ctx->tiny_num && ctx->nft_min_m >= 0 && M >= ctx->nft_min_m && M > 0;
    // numeric-first without the probe (short-row matrices below nft_min_m rows): every tiny row
    // is sorted once, in symbolic, into slots sized by the per-row bound
    nft_auto = !probe && M > 0 && ctx->nft_min_m >= 0 && M < ctx->nft_min_m && ctx->tiny_num && ctx->nft_slots &&
               ctx->nft_auto_avg > 0 && A->nnz < (long long)ctx->nft_auto_avg * M;
    // near row groups: with the row cache (their C patterns are compared there), not with
    // the numeric-first probe (big M), and union rows of at most 3 x 32 M values
    const bool near = ctx->near && ctx->groups && ctx->use_mcache && !probe && !nft_auto && A->nnz <= (1 << 25);
    const bool same_ab = A->ptr == B->ptr && A->col == B->col && A->val == B->val;
    L = plan(M, b.M, A->nnz, B->nnz, mc_list, -1, near, near && same_ab);
    const char* ws_before = ctx->ws;
    int rc = ensure(ctx, &ctx->ws, &ctx->ws_bytes, L.total);
    if (rc == MHS_ERR_OOM && near) {  // near groups are an optimisation: drop them before chunking
        (void)hipGetLastError();
        L = plan(M, b.M, A->nnz, B->nnz, mc_list, -1, false);
        rc = ensure(ctx, &ctx->ws, &ctx->ws_bytes, L.total);
    }
    if (rc == MHS_ERR_OOM && M > 1) return go_chunked();
    if (rc) return rc;
    if (ctx->ws != ws_before) ctx->stats_zero = false;
    if (ctx->poison >= 0) {  // MHS_POISON: every attempt finds its cached buffers as a workspace that has just grown
        MHS_HIP(poison_fill(ctx, ctx->ws, ctx->ws_bytes, s));
        MHS_HIP(poison_fill(ctx, ctx->gscratch, ctx->gscratch_bytes, s));
        MHS_HIP(poison_fill(ctx, ctx->slots, ctx->slots_bytes, s));
        ctx->stats_zero = false;  // (the device Stats went with them: the memset below follows)
    }
    const hipError_t e = pool_get(ctx, (void**)&own.out.ptr, (size_t)(M + 1) * 4);
    if (e == hipErrorOutOfMemory && M > 1) {
        (void)hipGetLastError();
        return go_chunked();
    }
    if (e != hipSuccess) return fail_hip(ctx, e, "allocating C.ptr");
    own.queued = true;  // (every step from here on queues work on C's arrays)
    w = make_work(ctx, L, M, A->nnz, B->nnz, mc_list);
    w.near_b = L.near && same_ab;
    if (L.near) {
        w.vcheck = B->val;
        w.vcheck_n = B->nnz;
    }
    // device Stats start zeroed: the previous call's k_scan left them so, else a memset
    if (!ctx->stats_zero) MHS_HIP(hipMemsetAsync(w.stats, 0, sizeof(Stats), s));
    ctx->stats_zero = false;  // until this call's k_scan has published and cleared them
    if (M == 0) MHS_HIP(hipMemsetAsync(own.out.ptr, 0, 4, s));
    t_alloc = ms_since(T0);
    if (t) MHS_HIP(hipEventRecord(ctx->ev[0], s));
    return MHS_OK;
}

// ---- Form_mask_matrix_B, symbolic_binning: the mask of B and k_analyze.  Numeric-first tiny
// rows (big M): k_analyze also bins the rows that way and counts them (the probe); the host
// picks the bin lists and sizes the candidates' value slots
int Call::analyze_rows() {
    fplan = plan_front_rows(front_shape());
    int i = 0;
    issue_upto(&i, FK_MASK);
    if (t) MHS_HIP(hipEventRecord(ctx->ev[1], s));
    auto slots = [&](size_t n) {  // the value slots of n entries, if they fit
        if (ensure(ctx, &ctx->slots, &ctx->slots_bytes, n * 12) != MHS_OK) return false;
        w.nft = 1;
        w.sc_val = (double*)ctx->slots;
        w.sc_col = (int*)(ctx->slots + n * 8);
        return true;
    };
    if (probe) w.nft_bin = (unsigned char*)(ctx->ws + L.nft_bin);
    if (nft_auto) {
        if (slots((size_t)M * TINY_SLOT_MAX)) w.nft_bin = (unsigned char*)(ctx->ws + L.nft_bin);
        else (void)hipGetLastError();
    }
    const int seq_probe = probe ? ++ctx->seq : 0;
    issue_upto(&i, FK_PROBE_PUBLISH, seq_probe);
    if (probe) {
        MHS_HIP(hipGetLastError());
        const int rc = wait_published(ctx, s, ctx->pub, seq_probe);
        if (rc) return rc;
        const unsigned long long n = ctx->pub->stats.an_slots;
        other = ctx->pub->stats.an_other;
        w.sym_big = other >= (1ull << 21);
        // slots pay where the tiny rows are (nearly) the whole product: elsewhere numeric's
        // tiny classes run beside the long rows' kernels anyway (measured: wb-edu-like +10%
        // with slots, 19% of its rows past the tiny classes; GAP-road- / delaunay-like -12% / -17%)
        if (!(n > 0 && ctx->nft_slots && other * 100 <= (unsigned long long)M * ctx->nft_other_pct && slots((size_t)n)))
            (void)hipGetLastError();
    }
    issue_upto(&i, FK_BIN_LIST);
    if (t) MHS_HIP(hipEventRecord(ctx->ev[2], s));
    return MHS_OK;
}

// ---- launch plan speculation (SpecArgs): the previous call's numeric plan on the same
// operands goes out right behind k_scan, checked on the device; not with the numeric-first
// probe (its own hand-off) or a forked symbolic pass
void Call::choose_plan() {
    const bool fork_big = ctx->sym_fork_min_m >= 0 && M >= ctx->sym_fork_min_m;
    fork_sym = ((w.nft && other > 0) || ctx->sym_fork || fork_big) && ctx->num_streams > 1 && ctx->aux[0];
    key = {{A->ptr, A->col, A->val, B->ptr, B->col, B->val}, M, b.N, b.M, A->nnz, B->nnz, ctx->gen,
           L.near, w.nft, mc_list, 0};
    plannable = ctx->spec && M > 0 && !probe && (!fork_sym || ctx->spec_fork);
    // (a plan dealt over several streams queues only its call-stream launches ahead of k_scan: see
    // NumPhase)
    spec = plannable && ctx->plan_valid && ctx->plan_key == key;
    ph = ctx->plan_h;
    // a speculated call whose plan has rows in the rare symbolic bins runs them on an aux stream
    // beside k_sym_common (their 38 us ran after it on scircuit-like); the plan left them out where
    // they were empty
    if (spec && !fork_sym && ctx->spec_fork_rare && ctx->num_streams > 1 && ctx->aux[0] &&
        (ph.sym_count[SYM_WM] > 0 || ph.sym_count[SYM_B1024] > 0 || ph.sym_count[SYM_GLOBAL] > 0))
        fork_sym = true;
    ctx->plan_valid = false;  // (set again by this call's success)
}

// ---- Calculate_C_nnz: the symbolic plan (plan_front_symbolic decides the launches, what a speculated
// plan leaves out and the order around the fork); here the fork event, the aux stream's wait ahead
// of its first launch -- behind the call stream's first: no host call ahead of that one -- and the join
int Call::launch_symbolic() {
    fplan = plan_front_symbolic(front_shape(), spec ? &ph : nullptr);
    // (a rerun does not speculate -- it leaves nothing out and adds nothing here)
    ctx->stat[MHS_STAT_SPEC_SKIPPED] += fplan.left_out;
    int fork = fplan.fork;  // 0: none; 1: forked; 2: the aux stream waits for the fork event; 3: joined
    if (fork) {
        ctx->stat[MHS_STAT_SYM_FORK] += !rerun;  // (once per user call: a miss has counted its first attempt)
        MHS_HIP(hipEventRecord(ctx->fork_ev, s));
    }
    auto advance = [&](int to) -> int {  // the fork's steps up to `to`, each once
        if (fork == 1 && to >= 2) {
            MHS_HIP(hipStreamWaitEvent(ctx->aux[0], ctx->fork_ev, 0));
            fork = 2;
        }
        if (fork == 2 && to >= 3) {
            MHS_HIP(hipEventRecord(ctx->join_ev[0], ctx->aux[0]));
            MHS_HIP(hipStreamWaitEvent(s, ctx->join_ev[0], 0));
            fork = 3;
        }
        return MHS_OK;
    };
    for (int i = 0; i <= fplan.n; ++i) {  // (past the last launch: what is left of the fork's steps)
        const FrontLaunch* l = i < fplan.n ? &fplan.launch[i] : nullptr;
        const int rc = advance(!l || l->after_join ? 3 : l->stream == FRONT_AUX ? 2 : 0);
        if (rc) return rc;
        if (l) issue(*l);
    }
    MHS_HIP(hipGetLastError());
    if (t) MHS_HIP(hipEventRecord(ctx->ev[3], s));
    return MHS_OK;
}

// ---- numeric_binning: scan, classify, bins.  k_scan publishes the Stats to pinned host
// memory (no rows: nothing to scan, the zeroed Stats are read back)
int Call::launch_scan() {
    if (M > 0) {
        seq = ++ctx->seq;
        const SpecArgs sa{ctx->d_go, ph};
        issue(front_scan(M), seq, spec ? &sa : nullptr);
        MHS_HIP(hipGetLastError());
    } else {
        MHS_HIP(hipGetLastError());
        MHS_HIP(hipMemcpyAsync(ctx->h_stats, w.stats, sizeof(Stats), hipMemcpyDeviceToHost, s));
    }
    if (t) MHS_HIP(hipEventRecord(ctx->ev[4], s));
    return MHS_OK;
}

// ---- Malloc_C_col_val for the numeric pass of `of` (this call's Stats, or the plan's): C.col /
// C.val, the global-bin scratch, and for near union runs of B (A*A, near groups verified) B's
// arrays copied in front of the union rows (in the near check instead, for every call with
// candidates: cant-perturbed-like -1.5 %, cant-s1-like symbolic +5 % -- candidates, no groups).
// *no_room: C's arrays (alloc_err says why; no message yet: the call may still succeed) or the
// scratch could not be had, and nothing was queued.
int Call::prepare_numeric(const Stats& of, bool* no_room) {
    *no_room = true;
    alloc_err = alloc_c(ctx, &own.out, of.nnzC);
    if (alloc_err != hipSuccess) return alloc_err == hipErrorOutOfMemory ? MHS_ERR_OOM : MHS_ERR_HIP;
    const int rc = ensure_gscratch(ctx, w, of);
    if (rc) return rc;
    *no_room = false;
    if (w.near_b && of.near_verified > 0 && B->nnz > 0) {
        MHS_HIP(hipMemcpyAsync(w.bx_col, B->col, (size_t)B->nnz * 4, hipMemcpyDeviceToDevice, s));
        MHS_HIP(hipMemcpyAsync(w.bx_val, B->val, (size_t)B->nnz * 8, hipMemcpyDeviceToDevice, s));
        w.bx_on = 1;
    }
    return MHS_OK;
}

// ---- Numeric: the launches of `of` in `phase`, or (an empty C) the ring's two events alone
int Call::run_or_stamp(const Stats& of, int phase) {
    own.out.nnz = (int)of.nnzC;
    if (of.nnzC > 0) return run_numeric(ctx, a, b, w, of, own.out, nplan, nev0, nev1, phase);
    if (nev0) {
        MHS_HIP(hipEventRecord(nev0, s));
        MHS_HIP(hipEventRecord(nev1, s));
    }
    return MHS_OK;
}

// Phase A of the previous call's plan, queued behind k_scan before its Stats are known.
int Call::speculate_numeric() {
    if (!spec) return MHS_OK;
    const auto T5 = std::chrono::steady_clock::now();
    bool no_room = ctx->spec_no_room;  // (MHS_SPEC_NO_ROOM, tests: the branch below without filling the device)
    int rc = no_room ? MHS_OK : prepare_numeric(ph, &no_room);
    if (no_room) {  // (no room for the plan's C: phase A stays in, finish_speculated decides what follows)
        own.give_back_cols();
        (void)hipGetLastError();
        return MHS_OK;
    }
    if (rc) return rc;
    t_malloc = ms_since(T5);
    if (t) MHS_HIP(hipEventRecord(ctx->ev[5], s));
    w.go = ctx->d_go;
    rc = run_or_stamp(ph, NUM_SPEC_A);
    if (rc) return rc;
    if (t) MHS_HIP(hipEventRecord(ctx->ev[6], s));
    launched = true;
    ++ctx->stat[MHS_STAT_SPEC];
    return MHS_OK;
}

// The one host round trip: the host spins on k_scan's sequence number (no stream sync, no
// interrupt wake-up) and copies the published Stats.
int Call::handoff() {
    if (M > 0) {
        const int rc = wait_published(ctx, s, ctx->pub, seq);
        if (rc) return rc;
        memcpy(&h, (const void*)&ctx->pub->stats, sizeof(Stats));
        ctx->stats_zero = true;  // k_scan's last block cleared them after publishing
    } else {
        MHS_HIP(hipStreamSynchronize(s));
        h = *ctx->h_stats;
    }
    return MHS_OK;
}

// What the hand-off makes of the call: spec_outcome (mhs_shape.hpp) decides, here and nowhere else.
// A hit: the plan's aux-stream launches and joins (phase B).  A rerun (the miss): every array is
// rewritten by a call without speculation -- also when phase A never went out, and when the Stats
// carry an error: a speculated call left symbolic launches out, so Stats that are not the plan's
// may hold stale counts, and the rerun reports a genuine error again.
int Call::finish_speculated() {
    outcome = spec_outcome(spec, launched, h.err != 0, spec && stats_same_plan(h, ph));
    switch (outcome) {
    case SPEC_PROCEED:
        return MHS_OK;
    case SPEC_HIT:
        ctx->stat[MHS_STAT_WIDE_OFFSETS] += ph.nnzC > 0 && !nplan.o32;  // (a miss: counted by the rerun)
        return ph.nnzC > 0 ? run_numeric(ctx, a, b, w, ph, own.out, nplan, nev0, nev1, NUM_SPEC_B) : MHS_OK;
    case SPEC_RERUN:
        break;
    }
    MHS_HIP(hipStreamSynchronize(s));
    own.give_back();
    ++ctx->stat[MHS_STAT_SPEC_MISS];  // (once per user call: the rerun does not speculate)
    return CALL_RERUN;  // (plan_valid is false: no speculation)
}

// The call's own Stats are final: the device-side checks, C's size, the path counters.  Then,
// unless a plan hit, the ordinary numeric phase sized by them; C beside the full workspace may
// not fit: the call then goes on with a row-chunked workspace.
int Call::numeric_after_handoff() {
    if (h.err) return fail_stats(ctx, h.err);
    own.out.nnz = (int)h.nnzC;
    ctx->stat[MHS_STAT_NFT] += w.nft != 0;
    ctx->stat[MHS_STAT_NEAR] += L.near && h.near_verified > 0;
    if (outcome == SPEC_HIT) return MHS_OK;
    const auto T5 = std::chrono::steady_clock::now();
    bool no_room = false;
    int rc = prepare_numeric(h, &no_room);
    if (no_room) {
        own.give_back();
        (void)hipGetLastError();
        if (rc == MHS_ERR_OOM && M > 1) return go_chunked();
        return alloc_err != hipSuccess ? fail_hip(ctx, alloc_err, "allocating C.col/C.val") : rc;
    }
    if (rc) return rc;
    t_malloc = ms_since(T5);
    if (t) MHS_HIP(hipEventRecord(ctx->ev[5], s));
    w.go = nullptr;
    rc = run_or_stamp(h, NUM_ALL);
    if (rc) return rc;
    ctx->stat[MHS_STAT_WIDE_OFFSETS] += h.nnzC > 0 && !nplan.o32;
    MHS_HIP(hipGetLastError());
    if (t) MHS_HIP(hipEventRecord(ctx->ev[6], s));
    return MHS_OK;
}

// The reference's per-phase times from the call's events (the stream has been synchronised).
int Call::fill_timing(mhs_timing& tm) {
    const int span[5] = {0, 1, 2, 3, 5};  // ev[i] .. ev[i + 1]
    float ms[5] = {};
    for (int i = 0; i < 5; ++i) MHS_HIP(hipEventElapsedTime(&ms[i], ctx->ev[span[i]], ctx->ev[span[i] + 1]));
    tm.mem_alloc = t_alloc;
    tm.Form_mask_matrix_B = ms[0];
    tm.symbolic_binning = ms[1];
    tm.Calculate_C_nnz = ms[2];
    tm.numeric_binning = ms[3];
    tm.Malloc_C_col_val = t_malloc;
    tm.Numeric = ms[4];
    tm.total_e2e = ms_since(T0);
    tm.total_ref = tm.total_e2e - tm.Form_mask_matrix_B;
    tm.flop = h.flop;
    tm.nnzC = h.nnzC;
    fill_bins(tm, M, h.sym_count, h.num_count);
    return MHS_OK;
}

// Stream sync (unless pipelined), the timing read-out, and only then the commit: C is the
// caller's and this call's Stats are the next call's plan.
int Call::finish_call() {
    ++ctx->ncalls;
    if (t || ctx->sync) MHS_HIP(hipStreamSynchronize(s));
    mhs_timing tm{};
    if (t) {
        const int rc = fill_timing(tm);
        if (rc) return rc;
        *t = tm;
    }
    own.commit(C);
    if (plannable) {  // the next call on these operands may speculate on this call's plan
        ctx->plan_key = key;
        ctx->plan_h = h;
        ctx->plan_valid = true;
    }
    return MHS_OK;
}

// One attempt at the call; CALL_RERUN after a speculation miss (`rerun`: the attempt that follows it).
int spgemm_attempt(mhs_ctx* ctx, const mhs_csr* A, const mhs_csr* B, mhs_csr* C, mhs_timing* t, bool rerun) {
    MHS_HIP(hipSetDevice(ctx->device));
    Call c(ctx, A, B, C, t, rerun);
    int rc = c.plan_workspace();
    if (rc == MHS_OK) rc = c.analyze_rows();
    if (rc == MHS_OK) c.choose_plan();
    if (rc == MHS_OK) rc = c.launch_symbolic();
    if (rc == MHS_OK) rc = c.launch_scan();
    if (rc == MHS_OK) rc = c.speculate_numeric();
    if (rc == MHS_OK) rc = c.handoff();
    if (rc == MHS_OK) rc = c.finish_speculated();
    if (rc == MHS_OK) rc = c.numeric_after_handoff();
    if (rc == MHS_OK) rc = c.finish_call();
    return rc == CALL_DONE ? MHS_OK : rc;
}

}  // namespace

extern "C" {

int mhs_abi_version(void) { return MHS_ABI_VERSION; }

int mhs_ctx_create(mhs_ctx** out, int device) {
    if (!out) return MHS_ERR_INVALID;
    *out = nullptr;
    mhs_ctx* ctx = new mhs_ctx();
    ctx->device = device;
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipHostMalloc((void**)&ctx->h_stats, sizeof(Stats), hipHostMallocDefault);
    if (e == hipSuccess)
        e = hipHostMalloc((void**)&ctx->pub, sizeof(Published), hipHostMallocMapped | hipHostMallocCoherent);
    if (e == hipSuccess) e = hipHostGetDevicePointer((void**)&ctx->d_pub, ctx->pub, 0);
    if (e == hipSuccess) memset(ctx->pub, 0, sizeof(Published));
    for (int i = 0; e == hipSuccess && i < 8; ++i) e = hipEventCreate(&ctx->ev[i]);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&ctx->stream_ev, hipEventDisableTiming);
    if (const char* v = getenv("MHS_NUM_STREAMS")) ctx->num_streams = std::max(1, std::min(atoi(v), mhs_ctx::NAUX + 1));
    if (e == hipSuccess) e = hipEventCreateWithFlags(&ctx->fork_ev, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&ctx->split_ev, hipEventDisableTiming);
    for (int i = 0; e == hipSuccess && i + 1 < ctx->num_streams; ++i) {
        e = hipStreamCreateWithFlags(&ctx->aux[i], hipStreamNonBlocking);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&ctx->join_ev[i], hipEventDisableTiming);
    }
    if (e == hipSuccess) e = hipMalloc((void**)&ctx->d_go, 256);
    if (e == hipSuccess) e = init_kernel_attributes();
    if (e == hipSuccess) e = hipDeviceGetAttribute(&ctx->cus, hipDeviceAttributeMultiprocessorCount, device);
    if (e != hipSuccess) {
        fprintf(stderr, "mhs_ctx_create: %s\n", hipGetErrorString(e));
        delete ctx;
        return e == hipErrorOutOfMemory ? MHS_ERR_OOM : MHS_ERR_HIP;
    }
    ctx->stream = ctx->own_stream;
    if (const char* e = getenv("MHS_DENSE_SPAN")) ctx->dense_span_max = atoi(e);
    if (getenv("MHS_NO_MCACHE")) ctx->use_mcache = false;
    if (const char* e = getenv("MHS_MC_LIST")) ctx->mc_list = atoi(e) < MC_LIST_MIN ? MC_LIST_MIN : atoi(e);
    if (getenv("MHS_NO_GROUPS")) ctx->groups = false;
    if (getenv("MHS_NO_NEAR")) ctx->near = false;
    if (getenv("MHS_NO_SPLIT")) ctx->split = false;
    if (getenv("MHS_NO_TINY_NUM")) ctx->tiny_num = false;
    if (const char* e = getenv("MHS_NFT_MIN_M")) ctx->nft_min_m = atoll(e);
    if (getenv("MHS_NFT_NO_SLOTS")) ctx->nft_slots = false;
    if (const char* e = getenv("MHS_SYM_FORK")) ctx->sym_fork = atoi(e) != 0;
    if (const char* e = getenv("MHS_SYM_FORK_MIN_M")) ctx->sym_fork_min_m = atoll(e);
    if (const char* e = getenv("MHS_NFT_OTHER_PCT")) ctx->nft_other_pct = atoi(e);
    if (const char* e = getenv("MHS_NFT_AUTO_AVG")) ctx->nft_auto_avg = atoi(e);
    if (const char* e = getenv("MHS_NO_SPEC")) ctx->spec = atoi(e) == 0;
    if (const char* e = getenv("MHS_SPEC_FORK")) {
        ctx->spec_fork = atoi(e) == 1;
        ctx->spec_fork_rare = atoi(e) == 2;
    }
    if (const char* e = getenv("MHS_GROUP_WALK"))
        if (atoi(e) == 0) ctx->cus = 0;
    if (const char* e = getenv("MHS_GROUP_GRID")) ctx->group_cap = std::max(0, atoi(e));  // (MHS_OPT_GROUP_GRID, A/B)
    if (const char* e = getenv("MHS_SPEC_NSS")) ctx->spec_nss = std::max(1, std::min(atoi(e), mhs_ctx::NAUX + 1));
    if (const char* e = getenv("MHS_SPEC_NO_ROOM")) ctx->spec_no_room = atoi(e) != 0;
    if (const char* e = getenv("MHS_NO_O32")) ctx->no_o32 = atoi(e) != 0;  // tests: the 64-bit-offset numeric kernels
    if (const char* e = getenv("MHS_POISON"))  // tests: a byte in every buffer a call did not write itself (poison_fill)
        if (*e && atoi(e) >= 0 && atoi(e) <= 255) ctx->poison = atoi(e);
    *out = ctx;
    return MHS_OK;
}

void mhs_ctx_destroy(mhs_ctx* ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    mhs_ctx_trim(ctx);  // outstanding C buffers belong to the caller
    if (ctx->stream_ev) (void)hipEventDestroy(ctx->stream_ev);
    if (ctx->fork_ev) (void)hipEventDestroy(ctx->fork_ev);
    if (ctx->split_ev) (void)hipEventDestroy(ctx->split_ev);
    for (int i = 0; i < mhs_ctx::NAUX; ++i) {
        if (ctx->aux[i]) {
            (void)hipStreamSynchronize(ctx->aux[i]);
            (void)hipStreamDestroy(ctx->aux[i]);
        }
        if (ctx->join_ev[i]) (void)hipEventDestroy(ctx->join_ev[i]);
    }
    if (ctx->h_stats) (void)hipHostFree(ctx->h_stats);
    if (ctx->pub) (void)hipHostFree(ctx->pub);
    for (auto& ev : ctx->nev)
        if (ev) (void)hipEventDestroy(ev);
    for (auto& ev : ctx->ev)
        if (ev) (void)hipEventDestroy(ev);
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->own_stream);
    if (ctx->d_go) (void)hipFree(ctx->d_go);
    delete ctx;
}

const char* mhs_last_error(const mhs_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int mhs_ctx_set_stream(mhs_ctx* ctx, void* s) {
    if (!ctx) return MHS_ERR_INVALID;
    hipStream_t next = s ? (hipStream_t)s : ctx->own_stream;
    if (next != ctx->stream) {
        // the workspace is shared by every call: work queued on the old stream (an
        // unsynchronised call's numeric phase) must finish before the new stream's
        // first kernel rewrites it
        MHS_HIP(hipSetDevice(ctx->device));
        MHS_HIP(hipEventRecord(ctx->stream_ev, ctx->stream));
        MHS_HIP(hipStreamWaitEvent(next, ctx->stream_ev, 0));
        ctx->stream = next;
    }
    return MHS_OK;
}

int mhs_ctx_fence_default_stream(mhs_ctx* ctx, int after) {
    if (!ctx) return MHS_ERR_INVALID;
    if (after != 0 && after != 1) return fail(ctx, MHS_ERR_INVALID, "mhs_ctx_fence_default_stream: after is 0 or 1");
    MHS_HIP(hipSetDevice(ctx->device));
    // (stream_ev: a wait already queued keeps the record it was queued behind, so the event can be recorded again)
    hipStream_t from = after ? ctx->stream : nullptr, to = after ? nullptr : ctx->stream;
    MHS_HIP(hipEventRecord(ctx->stream_ev, from));
    MHS_HIP(hipStreamWaitEvent(to, ctx->stream_ev, 0));
    return MHS_OK;
}

int mhs_ctx_trim(mhs_ctx* ctx) {
    if (!ctx) return MHS_ERR_INVALID;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    if (ctx->ws) (void)hipFree(ctx->ws);
    if (ctx->gscratch) (void)hipFree(ctx->gscratch);
    if (ctx->slots) (void)hipFree(ctx->slots);
    ctx->ws = ctx->gscratch = ctx->slots = nullptr;
    ctx->ws_bytes = ctx->gscratch_bytes = ctx->slots_bytes = 0;
    for (auto& b : ctx->pool) (void)hipFree(b.first);
    ctx->pool.clear();
    return MHS_OK;
}

void mhs_csr_free(mhs_csr* C) {
    if (!C) return;
    if (C->ptr) (void)hipFree(C->ptr);
    if (C->col) (void)hipFree(C->col);
    if (C->val) (void)hipFree(C->val);
    std::memset(C, 0, sizeof *C);
}

void mhs_ctx_recycle(mhs_ctx* ctx, mhs_csr* C) {
    if (!C) return;
    if (!ctx) {
        mhs_csr_free(C);
        return;
    }
    pool_put(ctx, C->ptr);
    pool_put(ctx, C->col);
    pool_put(ctx, C->val);
    std::memset(C, 0, sizeof *C);
}

int mhs_spgemm(mhs_ctx* ctx, const mhs_csr* A, const mhs_csr* B, mhs_csr* C, mhs_timing* t) {
    if (const int rc = check_args(ctx, A, B, C)) return rc;
    for (bool rerun = false;; rerun = true) {  // (a rerun finds plan_valid false: it cannot speculate, so cannot miss again)
        const int rc = spgemm_attempt(ctx, A, B, C, t, rerun);
        if (rc != CALL_RERUN) return rc;
    }
}

int mhs_transpose(mhs_ctx* ctx, const mhs_csr* A, mhs_csr* At) {
    if (!ctx || !A || !At) return fail(ctx, MHS_ERR_INVALID, "mhs_transpose: null argument");
    if (A->M < 0 || A->N < 0 || A->nnz < 0 || (A->M > 0 && !A->ptr) || (A->nnz > 0 && (!A->col || !A->val)))
        return fail(ctx, MHS_ERR_INVALID, "mhs_transpose: malformed A");
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return fail_hip(ctx, e, "hipSetDevice");
    const Csr a{A->M, A->N, A->nnz, A->ptr, A->col, A->val};
    size_t tmp_bytes = 0;
    e = transpose_csr(a, nullptr, nullptr, nullptr, nullptr, &tmp_bytes, ctx->stream);
    if (e != hipSuccess) return fail_hip(ctx, e, "transpose (scratch size)");
    mhs_csr T{A->N, A->M, A->nnz, nullptr, nullptr, nullptr};
    void* tmp = nullptr;
    e = hipMalloc((void**)&T.ptr, sizeof(int32_t) * ((size_t)A->N + 1));
    if (e == hipSuccess) e = hipMalloc((void**)&T.col, sizeof(int32_t) * (size_t)(A->nnz ? A->nnz : 1));
    if (e == hipSuccess) e = hipMalloc((void**)&T.val, sizeof(double) * (size_t)(A->nnz ? A->nnz : 1));
    if (e == hipSuccess) e = hipMalloc(&tmp, tmp_bytes ? tmp_bytes : 16);
    if (e == hipSuccess) e = poison_fill(ctx, T.ptr, sizeof(int32_t) * ((size_t)A->N + 1), ctx->stream);
    if (e == hipSuccess) e = poison_fill(ctx, T.col, sizeof(int32_t) * (size_t)(A->nnz ? A->nnz : 1), ctx->stream);
    if (e == hipSuccess) e = poison_fill(ctx, T.val, sizeof(double) * (size_t)(A->nnz ? A->nnz : 1), ctx->stream);
    if (e == hipSuccess) e = poison_fill(ctx, tmp, tmp_bytes ? tmp_bytes : 16, ctx->stream);
    if (e == hipSuccess) e = transpose_csr(a, T.ptr, T.col, T.val, tmp, &tmp_bytes, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (tmp) (void)hipFree(tmp);
    if (e != hipSuccess) {
        mhs_csr_free(&T);
        return fail_hip(ctx, e, "transpose");
    }
    *At = T;
    return MHS_OK;
}

int mhs_ctx_set_option(mhs_ctx* ctx, int option, int value) {
    if (!ctx) return MHS_ERR_INVALID;
    switch (option) {
    case MHS_OPT_SYNC:
        ctx->sync = value != 0;
        return MHS_OK;
    case MHS_OPT_NUMERIC_EVENTS: {
        if (value < 0 || value > 4096) return fail(ctx, MHS_ERR_INVALID, "numeric event ring size out of [0, 4096]");
        MHS_HIP(hipSetDevice(ctx->device));
        MHS_HIP(hipStreamSynchronize(ctx->stream));
        for (auto& ev : ctx->nev) (void)hipEventDestroy(ev);
        ctx->nev.assign(2 * (size_t)value, nullptr);
        for (auto& ev : ctx->nev) MHS_HIP(hipEventCreate(&ev));
        ctx->ncalls = 0;
        return MHS_OK;
    }
    case MHS_OPT_MEM_BUDGET:
        if (value < 0) return fail(ctx, MHS_ERR_INVALID, "memory budget must be >= 0 MiB");
        ctx->mem_budget = (size_t)value << 20;
        ++ctx->gen;  // (a speculated plan belongs to the options it was made under)
        return MHS_OK;
    case MHS_OPT_SPECULATE:
        ctx->spec = value != 0;
        ctx->plan_valid = false;
        return MHS_OK;
    case MHS_OPT_TINY_FIRST_ROWS:
        ctx->nft_min_m = value;
        ++ctx->gen;
        return MHS_OK;
    case MHS_OPT_GROUP_GRID:
        if (value < 0) return fail(ctx, MHS_ERR_INVALID, "grouped grid cap must be >= 0 blocks");
        ctx->group_cap = value;
        ++ctx->gen;
        return MHS_OK;
    default:
        return fail(ctx, MHS_ERR_INVALID, "unknown option");
    }
}

long long mhs_ctx_chunked_calls(const mhs_ctx* ctx) { return ctx ? ctx->chunked_calls : -1; }

long long mhs_ctx_stat(const mhs_ctx* ctx, int which) {
    if (!ctx || which < 0 || which > MHS_STAT_POISON_FILLS) return -1;
    return which == MHS_STAT_CHUNKED ? ctx->chunked_calls : ctx->stat[which];
}

int mhs_ctx_numeric_ms(mhs_ctx* ctx, float* out, int n) {
    if (!ctx || (!out && n > 0)) return -MHS_ERR_INVALID;
    const long long ring = (long long)ctx->nev.size() / 2;
    if (ring == 0) return 0;
    long long have = ctx->ncalls < ring ? ctx->ncalls : ring;
    if (n < have) have = n;
    for (long long i = 0; i < have; ++i) {
        const long long call = ctx->ncalls - have + i;
        const int slot = (int)(call % ring);
        if (hipEventSynchronize(ctx->nev[2 * slot + 1]) != hipSuccess) return -MHS_ERR_HIP;
        float f = 0;
        if (hipEventElapsedTime(&f, ctx->nev[2 * slot], ctx->nev[2 * slot + 1]) != hipSuccess) return -MHS_ERR_HIP;
        out[i] = f;
    }
    return (int)have;
}

int mhs_probe_conflicts(mhs_ctx* ctx, uint64_t* count) {
    if (!ctx || !count) return MHS_ERR_INVALID;
    unsigned long long* dev = nullptr;
    MHS_HIP(hipSetDevice(ctx->device));
    MHS_HIP(probe_counter(&dev));
    if (!dev) return fail(ctx, MHS_ERR_INVALID, "probe statistics need the MHS_PROBE_STATS=1 build (libmhspgemm_probe.so)");
    unsigned long long v = 0;
    MHS_HIP(hipMemcpyAsync(&v, dev, sizeof v, hipMemcpyDeviceToHost, ctx->stream));
    MHS_HIP(hipMemsetAsync(dev, 0, sizeof v, ctx->stream));
    MHS_HIP(hipStreamSynchronize(ctx->stream));
    *count = v;
    return MHS_OK;
}

int mhs_memcpy(mhs_ctx* ctx, void* dst, const void* src, size_t bytes, int kind) {
    if (!ctx) return MHS_ERR_INVALID;
    if (bytes == 0) return MHS_OK;
    hipMemcpyKind k = kind == 0 ? hipMemcpyHostToDevice : kind == 1 ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    MHS_HIP(hipSetDevice(ctx->device));
    MHS_HIP(hipMemcpyAsync(dst, src, bytes, k, ctx->stream));
    MHS_HIP(hipStreamSynchronize(ctx->stream));
    return MHS_OK;
}

int mhs_device_alloc(mhs_ctx* ctx, void** p, size_t bytes) {
    if (!ctx || !p) return MHS_ERR_INVALID;
    MHS_HIP(hipSetDevice(ctx->device));
    MHS_HIP(hipMalloc(p, bytes ? bytes : 16));
    return MHS_OK;
}

int mhs_device_free(mhs_ctx* ctx, void* p) {
    if (!ctx) return MHS_ERR_INVALID;
    if (p) MHS_HIP(hipFree(p));
    return MHS_OK;
}

int mhs_hbm_peak(mhs_ctx* ctx, size_t bytes, int iters, double* gbps) {
    if (!ctx) return MHS_ERR_INVALID;
    if (!gbps || iters <= 0 || bytes < (1u << 20))
        return fail(ctx, MHS_ERR_INVALID, "mhs_hbm_peak: needs gbps[3], iters > 0 and bytes >= 1 MiB");
    MHS_HIP(hipSetDevice(ctx->device));
    MHS_HIP(hbm_peak_run(bytes, iters, gbps));
    return MHS_OK;
}

}  // extern "C"
