// mhs_internal.hpp -- shared host/device declarations of the MI355X SpGEMM.
//
// Layout in HBM (all arrays live in the context workspace unless noted):
//   B side (per B row r, built by k_mask_b = Form_mask_matrix_B):
//     btcol[nnzB]  int32   tile column (col >> 6) of each 64-column tile of row r,
//     btmask[nnzB] uint64  bitmask of the row's columns inside that tile;
//                          row r's tiles sit at [B.ptr[r], B.ptr[r] + ntiles(r)),
//                          i.e. the tile arrays reuse B's own row_ptr (tiles(r) <= nnz(r)),
//                          so no scan and no second pass are needed.
//     bmeta[MB]    int4    {tile start (= B.ptr[r]), nnz(r), ntiles(r), lo tile}
//     bhi[MB]      int32   hi tile (lo = INT_MAX / hi = -1 for empty rows)
//   C side (per C row i, built by k_analyze):
//     rflop[M]  products of row i (saturated int32)   = the reference's "flop"
//     rtflop[M] tile products of row i               = the reference's "tile-flop"
//     rlo/rhi   tile span of row i
//     ctiles[M] distinct C tiles of row i (symbolic)
//     C.ptr     nnz of row i (symbolic), then scanned in place to the row_ptr
//   binning: bin id per row (uint8), per-block bin counts, row lists grouped by bin.
// The constants, bins, Stats and LDS needs are in mhs_shape.hpp, the pre-numeric launch plans in
// mhs_frontplan.hpp, the numeric launch plan in mhs_numplan.hpp (all HIP-free); this header adds what
// takes HIP types: the call's arrays, and issue_front / issue_numeric, which launch one plan entry.
#pragma once
#include <hip/hip_runtime.h>

#include "mhs_frontplan.hpp"
#include "mhs_numplan.hpp"

namespace mhs {

// ------------------------------------------------------------ launchers ---
struct Csr {
    int M, N, nnz;
    const int* ptr;
    const int* col;
    const double* val;
};

struct SpillLists;  // (mhs_kernels.hip) symbolic's tile lists of rows past the row-cache cap
struct SpillArea {
    unsigned long long* mask;
    int* key;
    int* lofs;
    int* top;
    long long cap;
};
// entries of the spill region: one per B nonzero (at least 1 M, at most 64 M = 768 MB)
inline long long spill_cap(long long nnzB) {
    const long long c = nnzB < (1LL << 20) ? (1LL << 20) : nnzB;
    return c > (1LL << 26) ? (1LL << 26) : c;
}

struct Work {
    // B side
    int* btcol;
    unsigned long long* btmask;
    int4* bmeta;
    int* bhi;
    // C side
    int* rflop;
    int* rtflop;
    int* rlo;
    int* rhi;
    int* ctiles;
    unsigned char* sym_bin;  // M: symbolic bin of every row (k_analyze)
    unsigned char* asame;    // M: row has the column pattern of row-1 (k_analyze)
    unsigned char* grp;      // M: row groups (k_bin_list; see RG_MAX)
    int groups;              // form row groups (0: every row alone)
    // near row groups (GRP_NEAR; nullptr: off): candidate list (head * 4 + R), union rows
    // at the head's A offset (ucol: nnz(A) ints; uval: 3 nnz(A) doubles, values of row r at
    // 3 * Aptr[head] + r * nU), union length per head
    int* near_list;
    unsigned* nsig;  // M: k_analyze's near-link signature of every row
    int* ucol;
    double* uval;
    int* gna;
    int near_b;      // B is A with near groups planned: k_scan marks the verified heads in bmeta
    // B's arrays extended by the near union rows (nnzB + 3 nnzA entries; uval = bx_val + nnzB,
    // ucolx = bx_col + nnzB): the numeric value walks read them when bx_on (B is A, groups verified)
    int* bx_col;
    double* bx_val;
    int* ucolx;
    int bx_on;
    const double* vcheck;    // B's values, checked for Inf / NaN by the near check (near groups planned)
    long long vcheck_n;
    int tiny_num;            // numeric tiny classes allowed (per row: column span <= TINY_NUM_NMAX + 1)
    // numeric-first tiny rows (big M): the symbolic tiny launch sorts them once, in the
    // numeric classes, and sums their values into slots (sc_*); numeric only copies them
    // into C.  nft_bin (M, the probe): k_analyze also bins every row that way and counts
    // the candidates; the host then picks the bin lists (nft: numeric-first, with slots).
    unsigned char* nft_bin;
    int nft;
    long long* tslot;        // M: a slot row's first entry
    int* sc_col;
    double* sc_val;
    int* bin_list;           // (NUM_NB-1) * M: bin x's rows at (x-1)*M (symbolic bins, then numeric bins)
    int* split_list;         // M: the block bins' rows split by LDS need (k_split_bins): B1024's, then B256's
    unsigned long long* blkflop;  // per-block flop partials of k_analyze
    int nflop;                    // their count
    int* scan_part;    // k_scan's look-back state: one 64-bit word per block (flag | prefix)
    int* cursors;      // CURSOR_INTS row cursors (after the look-back words), then BINCNT_INTS bin counters
    unsigned long long* mcache;   // [M][mc_stride] tile masks / tile lists (symbolic -> numeric)
    int mc_list;                  // list cap (see mlisted)
    SpillArea spill;              // tile lists of rows past mc_list (symbolic -> numeric)
    Stats* stats;
    void* gscratch;    // global-bin scratch
    size_t gscratch_bytes;
    const int* go;     // speculated numeric launches: run only when *go == 1 (k_scan's verdict); nullptr: always
    int sym_big;       // the numeric-first probe counted >= 2^21 rows past the tiny classes: big symbolic wave grid
};

// The arrays the pre-numeric launches read and write: the pointer half of a launch, where FrontLaunch
// is the shape half.  References: the call fills in its Work as the stages go (nft, the value slots).
struct FrontPointers {
    const Csr &A, &B;
    const Work& w;
    int* Cptr;
    int dense_span_max;
    Published* pub;  // where k_probe_publish and k_scan publish
};
// One launch of a call's pre-numeric plans (plan_front_rows, plan_front_symbolic, front_scan) on `s`.
// seq: what FK_PROBE_PUBLISH / FK_SCAN publish; spec: k_scan's check of a speculated plan (null: none).
void issue_front(const FrontLaunch& l, const FrontPointers& p, hipStream_t s, int seq = 0, const SpecArgs* spec = nullptr);
// The arrays a call's numeric launches read and write (and the two scalars the kernels take beside
// them): the pointer half of a launch, where NumLaunch is the shape half.  Built once per call.
struct NumPointers {
    Csr A, B;
    Work w;
    int* Cptr;
    int* Ccol;
    double* Cval;
    int dense_span_max;
};
// One launch of a call's plan (plan_numeric) on `s`.  start / stop (either may be null): events the
// dispatch packet itself carries (hipExtLaunchKernel) instead of records between the kernels.
void issue_numeric(const NumLaunch& l, bool o32, const NumPointers& p, hipStream_t s, hipEvent_t start,
                   hipEvent_t stop);
// Block bins holding rows on both sides of their LDS split: partition their lists into
// w.split_list (small rows first, hub rows last) on `s`.  False when no bin splits.
bool launch_split_bins(const Work& w, const Stats& h, int M, const int* Cptr, hipStream_t s, int dense_span_max);
size_t sym_global_bytes_per_block(int N);
// p[0..n) += off (row-chunked products: a chunk's row_ptr rebased to its place in C)
void launch_add_offset(int* p, int n, int off, hipStream_t s);
// Device CSR transpose (AAT operand): tmp == nullptr -> *tmp_bytes = scratch size.
hipError_t transpose_csr(const Csr& A, int* tptr, int* tcol, double* tval, void* tmp, size_t* tmp_bytes,
                         hipStream_t s);
// ... its pattern only, with the way back to A's values: trow[nnz] = the entry's row in A, tperm[nnz] = its
// position in A's arrays (a masked values plan's B^T).  The same sort, the same scratch.
hipError_t transpose_pattern(const Csr& A, int* tptr, int* trow, int* tperm, void* tmp, size_t* tmp_bytes,
                             hipStream_t s);
hipError_t init_kernel_attributes();
// mhs_values.hip: the values-only kernels' launch attributes (called by init_kernel_attributes; their
// declarations are in mhs_valwalk.hpp)
hipError_t init_values_attributes();
// device address of the probe-conflict counter (nullptr unless built with MHS_PROBE_STATS=1)
hipError_t probe_counter(unsigned long long** dev);
// mhs_hbm.hip: the streaming kernels of mhs_hbm_peak on the current device (gbps[3]: copy, read, write)
hipError_t hbm_peak_run(size_t bytes, int iters, double* gbps);

}  // namespace mhs
