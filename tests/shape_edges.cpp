// shape_edges.cpp -- derives the edge ladder of tests/test_gpu_edges.py from the shape headers.
//
// Every kernel family takes its rows by an LDS budget or a work cap of csrc/mhs_shape.hpp (full call) or
// csrc/mhs_valplan.hpp (values-only call and its backward).  This program restates the three bin ladders
// of mhs_kernels.hip (num_bin_of, num_group_bin_of, sym_bin_of) over the headers' own functions and
// constants, scans one parameter of a generated row family (tests/_util.py: edge_band, edge_scatter,
// edge_work, edge_symwork, edge_val) and prints, for every rung, the last parameter value that stays in a
// bin and the first that leaves it, with the row parameters and the bin on each side.  No threshold is
// written down here: a changed constant moves the rungs, and tests/test_shape_edges_host.py fails until
// tests/golden/shape_edges.json is regenerated from this program's output.
//
//   c++ -std=c++17 -Wall -Werror -I mh-spgemm_amd/csrc tests/shape_edges.cpp -o shape_edges && ./shape_edges
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <string>

#include "mhs_shape.hpp"
#include "mhs_valplan.hpp"

using namespace mhs;

namespace {

const char* const NUM_NAMES[NUM_NB] = {"NUM_NONE", "NUM_WS", "NUM_W16", "NUM_B256", "NUM_B1024", "NUM_GLOBAL", "NUM_WSG",
                                       "NUM_W16G", "NUM_TINY0", "NUM_TINY1", "NUM_TINY2", "NUM_TINY3", "NUM_TINY4",
                                       "NUM_TINY5", "NUM_WSH", "NUM_W16H"};
const char* const SYM_NAMES[SYM_NB] = {"SYM_NONE", "SYM_WAVE", "SYM_B256", "SYM_B1024", "SYM_GLOBAL", "SYM_TINY0",
                                       "SYM_TINY1", "SYM_TINY2", "SYM_TINY3", "SYM_TINY4", "SYM_TINY5", "SYM_WM"};
const char* const VAL_NAMES[VC_COUNT] = {"none", "team", "wave_direct", "wave_search", "block_direct", "block_search",
                                         "global"};
const char* const MODE_NAMES[3] = {"dense", "direct", "hash"};
static_assert(NUM_WSH == 14 && NUM_W16H == 15 && SYM_WM == 11, "the name tables follow the enums");

// One C row as the kernels see it: tile span, distinct tiles, C entries, products, tile products, A entries.
struct Row {
    int span, t, n, flop, tflop, nA;
};

// The rungs keep out of the register-sort classes, whose rule has a tuning constant outside the headers.
void no_tiny(const Row& r) {
    if (tiny_class(r.flop, r.nA) >= 0 || tiny_class_sym(r.flop, r.nA) >= 0) {
        fprintf(stderr, "a rung row fell into a tiny class: flop %d nA %d\n", r.flop, r.nA);
        exit(2);
    }
}

// num_bin_of (mhs_kernels.hip) for rows outside the tiny classes
int num_bin(const Row& r, int dsm) {
    if (r.n == 0) return NUM_NONE;
    const long long need = num_need(r.span, r.t, r.n, dsm);
    const bool hash = num_mode(r.span, r.t, r.n, dsm) == NM_HASH;
    if (need <= NUM_WS_BYTES - WAVE_HDR && r.flop <= NUM_WS_WORK) return hash ? NUM_WSH : NUM_WS;
    if (num_wide(r.span, r.t, r.n, dsm) || num_ranked(r.span, r.t, r.n, dsm)) return NUM_B1024;
    if (need <= NUM_W16_BYTES - WAVE_HDR && r.flop <= NUM_W16_WORK) return hash ? NUM_W16H : NUM_W16;
    if (need <= NUM_B256_BYTES - BLOCK_HDR && r.flop <= NUM_B256_WORK) return NUM_B256;
    if (need <= B1024_BYTES) return NUM_B1024;
    return NUM_GLOBAL;
}
// num_group_bin_of: the bin of a group of R rows (NUM_NONE: row by row)
int num_group_bin(const Row& r, int R, int dsm) {
    if (R < 2 || r.n == 0) return NUM_NONE;
    const long long need = num_need_rows(r.span, r.t, r.n, dsm, R);
    if (need <= NUM_WSG_BYTES - WAVE_HDR && r.flop <= NUM_WS_WORK) return NUM_WSG;
    if (need <= NUM_W16_BYTES - WAVE_HDR && r.flop <= NUM_W16_WORK) return NUM_W16G;
    return NUM_NONE;
}
// sym_bin_of
int sym_bin(const Row& r) {
    if (r.flop == 0) return SYM_NONE;
    const long long need = sym_need(r.span, r.tflop);
    if (need <= SYM_WAVE_BYTES - WAVE_HDR && r.tflop <= SYM_WAVE_WORK) return SYM_WAVE;
    if (need <= SYM_WM_BYTES - WAVE_HDR && r.tflop <= SYM_WAVE_WORK) return SYM_WM;
    if (need <= SYM_B256_BYTES - BLOCK_HDR && r.tflop <= SYM_B256_WORK) return SYM_B256;
    if (need <= B1024_BYTES) return SYM_B1024;
    return SYM_GLOBAL;
}

// The row families of tests/_util.py
Row band(int s, int n) { return Row{s, s, n, n, s, s}; }
Row scatter(int t, int n, int stride) { return Row{stride * (t - 1) + 1, t, n, n, t, t}; }
Row work(int flop) { return Row{1, 1, TILE_BITS, flop, flop / TILE_BITS + (flop % TILE_BITS ? 1 : 0), flop / TILE_BITS + (flop % TILE_BITS ? 1 : 0)}; }
Row symwork(int tflop) { return Row{1, 1, 1, tflop, tflop, tflop}; }

// The last x of [lo, hi) whose class is `from` while x + 1 has class `to`
int edge(int lo, int hi, const std::function<int(int)>& cls, int from, int to, const char* what) {
    for (int x = lo; x + 1 < hi; ++x)
        if (cls(x) == from && cls(x + 1) == to) return x;
    fprintf(stderr, "%s: no step from class %d to class %d in [%d, %d)\n", what, from, to, lo, hi);
    exit(2);
}

bool first_item = true;
void sep() {
    printf(first_item ? "\n" : ",\n");
    first_item = false;
}

std::string row_json(const Row& r) {
    char b[256];
    snprintf(b, sizeof b, "{\"span\": %d, \"t\": %d, \"n\": %d, \"flop\": %d, \"tflop\": %d, \"nA\": %d}", r.span, r.t, r.n,
             r.flop, r.tflop, r.nA);
    return b;
}

// One side of a rung of the full call.  `count`: which census entry it names ("num", "sym" or "" for result only).
void side(const char* key, const std::string& params, const Row& r, int dsm, int R, bool last) {
    no_tiny(r);
    const int gb = num_group_bin(r, R, dsm);
    const int nb = gb != NUM_NONE ? gb : num_bin(r, dsm);
    const long long need = R > 1 ? num_need_rows(r.span, r.t, r.n, dsm, R) : num_need(r.span, r.t, r.n, dsm);
    printf("      \"%s\": {\"params\": %s, \"row\": %s, \"mode\": \"%s\", \"num_need\": %lld, \"sym_need\": %lld, "
           "\"sym_direct\": %s, \"num_bin\": \"%s\", \"sym_bin\": \"%s\", \"grouped\": %s}%s\n",
           key, params.c_str(), row_json(r).c_str(), MODE_NAMES[num_mode(r.span, r.t, r.n, dsm)], need,
           sym_need(r.span, r.tflop), sym_direct(r.span, r.tflop) ? "true" : "false", NUM_NAMES[nb], SYM_NAMES[sym_bin(r)],
           gb != NUM_NONE ? "true" : "false", last ? "" : ",");
}

std::string fmt(const char* f, int a = 0, int b = 0, int c = 0) {
    char buf[160];
    snprintf(buf, sizeof buf, f, a, b, c);
    return buf;
}

void open_rung(const char* name, const char* family, const char* count, int dsm, int R) {
    sep();
    printf("    {\"name\": \"%s\", \"family\": \"%s\", \"count\": \"%s\", \"dense_span\": %d, \"R\": %d,\n", name, family, count,
           dsm, R);
}
void close_rung() { printf("    }"); }

// band(s, n), n scanned: numeric bins by LDS need (direct tables)
void band_rung(const char* name, int s, int from, int to) {
    const int lo = s > TINY_SLOT_MAX * 4 ? s : TINY_SLOT_MAX * 4 + 1;  // more than 512 products: no tiny class
    auto cls = [&](int n) { return num_bin(band(s, n), 0); };
    const int n = edge(lo, s * TILE_BITS + 1, cls, from, to, name);
    open_rung(name, "band", "num", 0, 1);
    side("last", fmt("{\"s\": %d, \"n\": %d}", s, n), band(s, n), 0, 1, false);
    side("first", fmt("{\"s\": %d, \"n\": %d}", s, n + 1), band(s, n + 1), 0, 1, true);
    close_rung();
}
// scatter(t, n, stride), n scanned: numeric bins by LDS need (hashed tables)
void scatter_rung(const char* name, int t, int stride, int from, int to) {
    auto cls = [&](int n) { return num_bin(scatter(t, n, stride), 0); };
    const int n = edge(t, t * TILE_BITS + 1, cls, from, to, name);
    open_rung(name, "scatter", "num", 0, 1);
    side("last", fmt("{\"t\": %d, \"n\": %d, \"stride\": %d}", t, n, stride), scatter(t, n, stride), 0, 1, false);
    side("first", fmt("{\"t\": %d, \"n\": %d, \"stride\": %d}", t, n + 1, stride), scatter(t, n + 1, stride), 0, 1, true);
    close_rung();
}

int val_cls(int n, int span, int P) { return val_class(n, span, P); }
void val_side(const char* key, int n, int span, int P, bool last) {
    printf("      \"%s\": {\"params\": {\"n\": %d, \"span\": %d, \"products\": %d}, \"class\": \"%s\", \"class_index\": %d, "
           "\"need\": %d}%s\n",
           key, n, span, P, VAL_NAMES[val_cls(n, span, P)], val_cls(n, span, P), val_row_need(val_cls(n, span, P), n, span),
           last ? "" : ",");
}
// x scanned; row(x) -> (n, span, products)
void val_rung(const char* name, int lo, int hi, const std::function<void(int, int&, int&, int&)>& row, int from, int to) {
    auto cls = [&](int x) {
        int n, span, P;
        row(x, n, span, P);
        return val_cls(n, span, P);
    };
    const int x = edge(lo, hi, cls, from, to, name);
    sep();
    printf("    {\"name\": \"%s\",\n", name);
    int n, span, P;
    row(x, n, span, P);
    val_side("last", n, span, P, false);
    row(x + 1, n, span, P);
    val_side("first", n, span, P, true);
    printf("    }");
}

}  // namespace

int main() {
    printf("{\n");
    printf("  \"constants\": {\"NUM_WS\": %d, \"NUM_W16\": %d, \"NUM_WSG\": %d, \"NUM_B256\": %d, \"B1024\": %d, \"SYM_WAVE\": %d, "
           "\"SYM_WM\": %d, \"SYM_B256\": %d, \"NUM_WS_WORK\": %d, \"NUM_W16_WORK\": %d, \"NUM_B256_WORK\": %d, "
           "\"SYM_WAVE_WORK\": %d, \"SYM_B256_WORK\": %d, \"HASH_CNT_T\": %d, \"STAGE_256\": %d, \"STAGE_1024\": %d, "
           "\"SCAN_ITEMS\": %d, \"WPB\": %d},\n",
           NUM_WS_BYTES - WAVE_HDR, NUM_W16_BYTES - WAVE_HDR, NUM_WSG_BYTES - WAVE_HDR, NUM_B256_BYTES - BLOCK_HDR, B1024_BYTES,
           SYM_WAVE_BYTES - WAVE_HDR, SYM_WM_BYTES - WAVE_HDR, SYM_B256_BYTES - BLOCK_HDR, NUM_WS_WORK, NUM_W16_WORK,
           NUM_B256_WORK, SYM_WAVE_WORK, SYM_B256_WORK, HASH_CNT_T, STAGE_SUBS * 64, STAGE_SUBS_1024 * 64, SCAN_ITEMS, WPB);
    printf("  \"num_bins\": {");
    for (int i = 0; i < NUM_NB; ++i) printf("%s\"%s\": %d", i ? ", " : "", NUM_NAMES[i], i);
    printf("},\n  \"sym_bins\": {");
    for (int i = 0; i < SYM_NB; ++i) printf("%s\"%s\": %d", i ? ", " : "", SYM_NAMES[i], i);
    printf("},\n");

    // ------------------------------------------------------------------ numeric rungs ---
    printf("  \"numeric\": [");
    first_item = true;
    band_rung("band10_ws_w16", 10, NUM_WS, NUM_W16);
    band_rung("band20_w16_b256", 20, NUM_W16, NUM_B256);
    band_rung("band120_b256_b1024", 120, NUM_B256, NUM_B1024);
    band_rung("band300_b1024_global", 300, NUM_B1024, NUM_GLOBAL);
    scatter_rung("scatter100_wsh_w16h", 100, 10, NUM_WSH, NUM_W16H);
    scatter_rung("scatter193_w16h_b256", HASH_CNT_T + 1, 10, NUM_W16H, NUM_B256);
    scatter_rung("scatter1500_b256_ranked", 1500, 10, NUM_B256, NUM_B1024);
    {  // ranked | wide windows: the stride (so the span) scanned; both in the 1024-thread bin
        const int t = 1500, n = 3100;
        auto cls = [&](int st) { return num_ranked(scatter(t, n, st).span, t, n, 0) ? 1 : num_wide(scatter(t, n, st).span, t, n, 0) ? 2 : 0; };
        const int st = edge(10, 2000, cls, 1, 2, "ranked_wide");
        open_rung("scatter1500_ranked_wide", "scatter", "", 0, 1);
        side("last", fmt("{\"t\": %d, \"n\": %d, \"stride\": %d}", t, n, st), scatter(t, n, st), 0, 1, false);
        side("first", fmt("{\"t\": %d, \"n\": %d, \"stride\": %d}", t, n, st + 1), scatter(t, n, st + 1), 0, 1, true);
        close_rung();
    }
    {  // count rank | bitonic rank of a hash row's tiles: t scanned; one bin
        const int n = 400, stride = 10;
        auto cls = [&](int t) { return hash_sort_p(t) == 0 ? 1 : 2; };
        const int t = edge(TILE_BITS + 1, n, cls, 1, 2, "count_bitonic");
        open_rung("scatter_count_bitonic", "scatter", "", 0, 1);
        side("last", fmt("{\"t\": %d, \"n\": %d, \"stride\": %d}", t, n, stride), scatter(t, n, stride), 0, 1, false);
        side("first", fmt("{\"t\": %d, \"n\": %d, \"stride\": %d}", t + 1, n, stride), scatter(t + 1, n, stride), 0, 1, true);
        close_rung();
    }
    for (int R = 2; R <= RG_MAX; ++R) {  // R identical consecutive band rows: grouped | row by row
        // (R = 3: three accumulators of more than 512 entries fit no grouped bin, so more than 64 A entries)
        const int s = R == 2 ? 10 : TILE_BITS + 6;
        auto cls = [&](int n) { return num_group_bin(band(s, n), R, 0); };
        const int lo = R == 2 ? TINY_SLOT_MAX * 4 + 1 : s;
        const int n = edge(lo, s * TILE_BITS + 1, cls, NUM_WSG, NUM_NONE, "group");
        open_rung(R == 2 ? "group2_wsg" : "group3_wsg", "band", "num", 0, R);
        side("last", fmt("{\"s\": %d, \"n\": %d}", s, n), band(s, n), 0, R, false);
        side("first", fmt("{\"s\": %d, \"n\": %d}", s, n + 1), band(s, n + 1), 0, R, true);
        close_rung();
    }
    {  // by work: work(flop), one 64-entry accumulator whatever the product count
        const struct {
            const char* name;
            int from, to;
        } W[3] = {{"work_ws_w16", NUM_WS, NUM_W16}, {"work_w16_b256", NUM_W16, NUM_B256}, {"work_b256_b1024", NUM_B256, NUM_B1024}};
        for (const auto& w : W) {
            auto cls = [&](int f) { return num_bin(work(f), 0); };
            const int f = edge(TILE_BITS * (TILE_BITS + 1), NUM_B256_WORK + TILE_BITS, cls, w.from, w.to, w.name);
            open_rung(w.name, "work", "num", 0, 1);
            side("last", fmt("{\"flop\": %d}", f), work(f), 0, 1, false);
            side("first", fmt("{\"flop\": %d}", f + 1), work(f + 1), 0, 1, true);
            close_rung();
        }
    }
    {  // by stage: block-bin band rows with one A entry fewer than, exactly, and one more than a stage
        const struct {
            int stage, bin;
            const char* name;
        } S[2] = {{STAGE_SUBS * 64, NUM_B256, "stage256"}, {STAGE_SUBS_1024 * 64, NUM_B1024, "stage1024"}};
        for (const auto& st : S)
            for (int d = -1; d <= 1; d += 2) {
                // n: the middle of the bin's range for s = stage (the same n on all three rows)
                auto cls = [&](int n) { return num_bin(band(st.stage + 1, n), 0); };
                const int n0 = edge(st.stage + 1, (st.stage - 1) * TILE_BITS, cls, st.bin - 1, st.bin, st.name) + 1;
                const int n1 = edge(st.stage + 1, (st.stage - 1) * TILE_BITS, cls, st.bin, st.bin + 1, st.name);
                const int n = (n0 + n1) / 2;
                const int s0 = d < 0 ? st.stage - 1 : st.stage, s1 = s0 + 1;
                open_rung((std::string(st.name) + (d < 0 ? "_below" : "_above")).c_str(), "band", "num", 0, 1);
                side("last", fmt("{\"s\": %d, \"n\": %d}", s0, n), band(s0, n), 0, 1, false);
                side("first", fmt("{\"s\": %d, \"n\": %d}", s1, n), band(s1, n), 0, 1, true);
                close_rung();
            }
    }
    printf("\n  ],\n");

    // -------------------------------------------- dense accumulators (MHS_DENSE_SPAN) ---
    printf("  \"dense\": [");
    first_item = true;
    {
        const int dsm = 512, per = 60;  // band(s, 60 s) under a context that takes spans up to 512 tiles dense
        const struct {
            const char* name;
            int from, to;
        } D[4] = {{"dense_ws_w16", NUM_WS, NUM_W16},
                  {"dense_w16_b256", NUM_W16, NUM_B256},
                  {"dense_b256_b1024", NUM_B256, NUM_B1024},
                  {"dense_b1024_global", NUM_B1024, NUM_GLOBAL}};
        for (const auto& d : D) {
            auto cls = [&](int s) { return num_bin(band(s, per * s), dsm); };
            const int s = edge(TINY_SLOT_MAX * 4 / per + 1, dsm + 1, cls, d.from, d.to, d.name);
            if (num_need(s, s, per * s, dsm) != num_need_dense(s)) return 3;
            open_rung(d.name, "band", "", dsm, 1);
            side("last", fmt("{\"s\": %d, \"n\": %d}", s, per * s), band(s, per * s), dsm, 1, false);
            side("first", fmt("{\"s\": %d, \"n\": %d}", s + 1, per * (s + 1)), band(s + 1, per * (s + 1)), dsm, 1, true);
            close_rung();
        }
    }
    printf("\n  ],\n");

    // ----------------------------------------------------------------- symbolic rungs ---
    printf("  \"symbolic\": [");
    first_item = true;
    {
        const struct {
            const char* name;
            int from, to;
        } B[4] = {{"symband_wave_wm", SYM_WAVE, SYM_WM},
                  {"symband_wm_b256", SYM_WM, SYM_B256},
                  {"symband_b256_b1024", SYM_B256, SYM_B1024},
                  {"symband_b1024_global", SYM_B1024, SYM_GLOBAL}};
        for (const auto& b : B) {  // band, one column per tile: direct-mapped masks over the span
            auto cls = [&](int s) { return sym_bin(band(s, s)); };
            const int s = edge(TINY_SLOT_MAX * 4 + 1, LDS_MAX / 4, cls, b.from, b.to, b.name);
            open_rung(b.name, "band", "sym", 0, 1);
            side("last", fmt("{\"s\": %d, \"n\": %d}", s, s), band(s, s), 0, 1, false);
            side("first", fmt("{\"s\": %d, \"n\": %d}", s + 1, s + 1), band(s + 1, s + 1), 0, 1, true);
            close_rung();
        }
    }
    {  // scatter, one column per tile, a wide stride: hashed masks and keys
        const int stride = 10;
        auto cls = [&](int t) { return sym_direct(scatter(t, t, stride).span, t) ? -1 : sym_bin(scatter(t, t, stride)); };
        const int t = edge(TILE_BITS + 1, 2000, cls, SYM_WAVE, SYM_WM, "symscatter");
        open_rung("symscatter_wave_wm", "scatter", "sym", 0, 1);
        side("last", fmt("{\"t\": %d, \"n\": %d, \"stride\": %d}", t, t, stride), scatter(t, t, stride), 0, 1, false);
        side("first", fmt("{\"t\": %d, \"n\": %d, \"stride\": %d}", t + 1, t + 1, stride), scatter(t + 1, t + 1, stride), 0, 1, true);
        close_rung();
    }
    {  // by work: one-entry B rows
        const struct {
            const char* name;
            int from, to;
        } W[2] = {{"symwork_wave_b256", SYM_WAVE, SYM_B256}, {"symwork_b256_b1024", SYM_B256, SYM_B1024}};
        for (const auto& w : W) {
            auto cls = [&](int tf) { return sym_bin(symwork(tf)); };
            const int tf = edge(TINY_SLOT_MAX * 4 + 1, SYM_B256_WORK + TILE_BITS, cls, w.from, w.to, w.name);
            open_rung(w.name, "symwork", "sym", 0, 1);
            side("last", fmt("{\"tflop\": %d}", tf), symwork(tf), 0, 1, false);
            side("first", fmt("{\"tflop\": %d}", tf + 1), symwork(tf + 1), 0, 1, true);
            close_rung();
        }
    }
    printf("\n  ],\n");

    // ------------------------------------------------------------- values-plan rungs ---
    printf("  \"values\": [");
    first_item = true;
    const int far = 2 * VAL_BLOCK_DIRECT_SPAN;                   // a span no direct table holds
    const int mid = VAL_TEAM_PMAX + (VAL_WAVE_PMAX - VAL_TEAM_PMAX) / 16;  // products of a wave row
    val_rung("team_n", 2, 4 * VAL_TEAM_NMAX, [&](int x, int& n, int& span, int& P) { n = x, span = 4 * VAL_TEAM_NMAX, P = 4 * VAL_TEAM_NMAX; },
             VC_TEAM, VC_WAVE_DIRECT);
    val_rung("team_products", VAL_TEAM_NMAX, 4 * VAL_TEAM_PMAX,
             [&](int x, int& n, int& span, int& P) { n = VAL_TEAM_NMAX, span = VAL_TEAM_NMAX, P = x; }, VC_TEAM, VC_WAVE_DIRECT);
    val_rung("wave_products", VAL_TEAM_PMAX + 1, 4 * VAL_WAVE_PMAX,
             [&](int x, int& n, int& span, int& P) { n = VAL_TEAM_NMAX, span = VAL_TEAM_NMAX, P = x; }, VC_WAVE_DIRECT,
             VC_BLOCK_DIRECT);
    val_rung("wave_span_to_block", 100, 4 * VAL_WAVE_DIRECT_SPAN, [&](int x, int& n, int& span, int& P) { n = 100, span = x, P = mid; },
             VC_WAVE_DIRECT, VC_BLOCK_DIRECT);
    val_rung("wave_span_to_search", 60, 4 * VAL_WAVE_DIRECT_SPAN, [&](int x, int& n, int& span, int& P) { n = 60, span = x, P = mid; },
             VC_WAVE_DIRECT, VC_WAVE_SEARCH);
    val_rung("wave_search_n", 100, 4 * VAL_WAVE_SEARCH_N, [&](int x, int& n, int& span, int& P) { n = x, span = far, P = x + 10; },
             VC_WAVE_SEARCH, VC_BLOCK_SEARCH);
    val_rung("block_span", 2 * VAL_WAVE_SEARCH_N, far,
             [&](int x, int& n, int& span, int& P) { n = 2 * VAL_WAVE_SEARCH_N, span = x, P = 2 * VAL_WAVE_PMAX; }, VC_BLOCK_DIRECT,
             VC_BLOCK_SEARCH);
    val_rung("block_search_n", 2 * VAL_WAVE_SEARCH_N, far, [&](int x, int& n, int& span, int& P) { n = x, span = far, P = x + 10; },
             VC_BLOCK_SEARCH, VC_GLOBAL);
    val_rung("dense_ratio", VAL_WAVE_DIRECT_SPAN + 1, 4 * VAL_WAVE_DIRECT_SPAN,
             [&](int x, int& n, int& span, int& P) { n = 100, span = x, P = mid; }, VC_BLOCK_DIRECT, VC_WAVE_SEARCH);
    printf("\n  ]\n}\n");
    return 0;
}
