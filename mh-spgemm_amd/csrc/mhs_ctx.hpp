// mhs_ctx.hpp -- the context behind the C ABI's mhs_ctx handle and the error helpers of the entry
// points, private to the library's host files: mhs_api.cpp (the SpGEMM call and the context's own
// entry points) and mhs_values_api.cpp (values plans and their calls).
#pragma once
#include "mhs_internal.hpp"
#include "../../include/mhspgemm.h"

#include <cstring>
#include <string>
#include <utility>
#include <vector>

struct mhs_ctx {
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    std::string err;
    char* ws = nullptr;
    size_t ws_bytes = 0;
    char* gscratch = nullptr;
    size_t gscratch_bytes = 0;
    mhs::Stats* h_stats = nullptr;  // pinned
    mhs::Published* pub = nullptr;  // fine-grained pinned: Stats handed over by the last pre-numeric kernel
    mhs::Published* d_pub = nullptr;
    int seq = 0;
    hipEvent_t ev[8] = {};
    bool sync = true;      // MHS_OPT_SYNC
    bool groups = true;     // row groups (MHS_NO_GROUPS=1: every row alone)
    bool near = true;       // near row groups (GRP_NEAR; MHS_NO_NEAR=1: off)
    bool split = true;      // block bins split by LDS need (MHS_NO_SPLIT=1: off)
    // MHS_OPT_NUMERIC_EVENTS: ring of (start, end) events around the numeric phase
    std::vector<hipEvent_t> nev;
    long long ncalls = 0;
    int mc_list = 0;         // tile-list cap of the row cache (0: mc_list_for(M); MHS_MC_LIST)
    bool stats_zero = false; // the workspace's device Stats are zero (left so by the last k_scan)
    bool use_mcache = true;  // symbolic keeps narrow rows' tile masks for numeric (MHS_NO_MCACHE)
    bool tiny_num = true;    // numeric tiny (sort) classes (MHS_NO_TINY_NUM=1: off)
    // numeric-first tiny rows from this many rows of A on (MHS_OPT_TINY_FIRST_ROWS,
    // MHS_NFT_MIN_M; < 0: never): one hand-off more per call, so big matrices only
    long long nft_min_m = 1 << 19;
    bool sym_fork = false;   // MHS_SYM_FORK=1: rare symbolic bins on an aux stream for every call
    // ... and for every call of at least this many rows (MHS_SYM_FORK_MIN_M; < 0: never): the
    // fork's cross-stream wait (~20 us) is noise there, the rare bins' milliseconds are not
    long long sym_fork_min_m = 1 << 19;
    bool nft_slots = true;   // MHS_NFT_NO_SLOTS=1 (tests): count the rows only, as when the slots do not fit
    int nft_other_pct = 5;   // slots only when at most this share of the rows is past the tiny classes (MHS_NFT_OTHER_PCT)
    // numeric-first tiny rows without the probe below nft_min_m rows, for matrices averaging fewer
    // than this many entries a row (MHS_NFT_AUTO_AVG; 0: off): the slots are sized by their upper
    // bound (TINY_SLOT_MAX a row), so no hand-off decides them
    int nft_auto_avg = 12;
    char* slots = nullptr;   // their value slots (cached across calls)
    size_t slots_bytes = 0;
    size_t mem_budget = 0;   // MHS_OPT_MEM_BUDGET (MiB): a call's workspace + C beyond it count as OOM (tests)
    size_t c_held = 0;       // C bytes a row-chunked call holds while it lays out its second pass
    long long front_passes = 0;  // front_pass calls (row-chunked passes; mhs_ctx_chunked_calls diagnostics)
    long long chunked_calls = 0;  // calls that ran row-chunked (mhs_ctx_chunked_calls)
    long long stat[11] = {};       // path counters (mhs_ctx_stat; [0] unused: chunked_calls)
    int dense_span_max = 0;  // NM_DENSE for rows spanning <= this many 64-column tiles (MHS_DENSE_SPAN; off: occupancy)
    // output pool (caching allocator for C arrays): (buffer, allocation size)
    std::vector<std::pair<void*, size_t>> pool;
    hipEvent_t stream_ev = nullptr;  // orders a new caller stream after the previous one
    // numeric bins on several streams (MHS_NUM_STREAMS, default 4; 1 = one stream): aux
    // streams fork from the call's stream after the Stats hand-off and join it before return
    static constexpr int NAUX = 7;
    int num_streams = 4;
    hipStream_t aux[NAUX] = {};
    hipEvent_t fork_ev = nullptr, join_ev[NAUX] = {};
    hipEvent_t split_ev = nullptr;  // k_split_bins done (the split block launches wait for it)
    // launch plan speculation (SpecArgs, mhs_shape.hpp): the last hand-off's Stats and the
    // operands they belong to; MHS_NO_SPEC=1 turns it off
    struct PlanKey {
        const void* p[6];
        long long M, N, MB, nnzA, nnzB, gen;
        int near, nft, mc_list, pad;  // (no implicit padding: compared bytewise)
        bool operator==(const PlanKey& o) const { return memcmp(this, &o, sizeof *this) == 0; }
    };
    bool spec = true;
    bool plan_valid = false;
    PlanKey plan_key{};
    mhs::Stats plan_h{};
    long long gen = 0;        // bumped by every mhs_ctx_set_option (options change the pipeline)
    int* d_go = nullptr;      // k_scan's verdict on a speculated plan (device int)
    bool spec_fork = false;  // MHS_SPEC_FORK=1: speculated plans also behind every forked symbolic pass (A/B)
    // speculated calls run their plan's rare symbolic rows on an aux stream beside k_sym_common
    // (scircuit-like -3.9 %, the other configs within 0.5 %: r06sf2); MHS_SPEC_FORK=0 turns it off
    bool spec_fork_rare = true;
    int spec_nss = mhs_ctx::NAUX + 1;  // streams of a speculated numeric phase (MHS_SPEC_NSS: a cap, A/B)
    // MHS_SPEC_NO_ROOM=1 (tests): a speculated call behaves as if the plan's C had not fitted -- its phase A
    // stays in (a budget cannot force that: the first call's C fitted under it); other calls are not touched
    bool spec_no_room = false;
    // MHS_NO_O32=1 (tests): every numeric plan takes the 64-bit-offset kernels, which the size rule of
    // plan_numeric selects only from 2^29 entries of B on (MHS_STAT_WIDE_OFFSETS counts the calls)
    bool no_o32 = false;
    // MHS_POISON=<byte> (tests; -1: off): poison_fill() below fills with this byte every device buffer the library
    // allocates for its own work, every buffer the output pool hands out and, at the start of every attempt of
    // mhs_spgemm, the cached workspace, global-bin scratch and value slots (MHS_STAT_POISON_FILLS counts the fills)
    int poison = -1;
    // the grouped numeric bin's cursor walk (plan_numeric): the device's compute units size its
    // resident set (MHS_GROUP_WALK=0: cus stays 0, the static walk); MHS_OPT_GROUP_GRID caps its blocks
    int cus = 0;
    int group_cap = 0;
};

namespace mhs {

// An entry point's failure: the message is kept for mhs_last_error, the code returned.
inline int fail(mhs_ctx* ctx, int code, const std::string& what) {
    if (ctx) ctx->err = what;
    return code;
}

inline int fail_hip(mhs_ctx* ctx, hipError_t e, const char* what) {
    std::string m = std::string(what) + ": " + hipGetErrorString(e);
    (void)hipGetLastError();
    return fail(ctx, e == hipErrorOutOfMemory ? MHS_ERR_OOM : MHS_ERR_HIP, m);
}

// (in a function that returns an error code and has the context as `ctx`)
#define MHS_HIP(expr)                                                   \
    do {                                                                \
        hipError_t e_ = (expr);                                         \
        if (e_ != hipSuccess) return fail_hip(ctx, e_, #expr);          \
    } while (0)

inline size_t al(size_t x) { return (x + 255) & ~size_t(255); }

// MHS_POISON: `bytes` of the library's own buffer `p` filled with the context's poison byte on `s`, the stream
// its next consumer runs on.  Off (the default): one branch.
inline hipError_t poison_fill(mhs_ctx* ctx, void* p, size_t bytes, hipStream_t s) {
    if (ctx->poison < 0 || !p || bytes == 0) return hipSuccess;
    ++ctx->stat[MHS_STAT_POISON_FILLS];
    return hipMemsetAsync(p, ctx->poison, bytes, s);
}

}  // namespace mhs
