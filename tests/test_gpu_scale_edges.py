"""GPU tests of the full call (mhs_spgemm) where a quantity nears 2^31 or 2^32, and of the numeric kernels that
only huge operands select -- all at shapes of a few MB.

A. The 64-bit-offset numeric kernels.  plan_numeric gives every table kernel 32-bit byte offsets into B's arrays
   while nnz(B) + 3 nnz(A) < 2^29; the twins for larger operands (twelve kernels, TWINS below) run here on the
   suite's own cases, on contexts created with MHS_NO_O32=1: every entry of tests/test_gpu_f64_bound.py's
   FULL_CALLS and the row-chunked perturbed_fem of tests/test_gpu_nonfinite.py, judged as there (pattern bit-exact
   against the oracle, values within 1.01 m 2^-53 S of long-double sums, the entry's census), plus the smallest inputs for
   the kernels those leave out: copy_zoo (the slot copy fused with the small hash bin, at each lane count) and
   wave16_zoo (the two 10 KiB wave bins).  MHS_STAT_WIDE_OFFSETS counts
   the calls; test_every_twin_ran names the case that launches each kernel.
B. nnz(C) at INT32_MAX (not an overflow: C does not fit the budget) and one past it (MHS_ERR_OVERFLOW from k_scan's
   verdict, from the row-chunked total, and from the rerun of a speculated call), each followed by correct calls
   on the same context and no device memory kept.
C. Columns up to 2^31 - 2, the tile of the kernels' INT_MAX column sentinel: the five A x B zoos shifted to the
   top of an N = INT32_MAX column space, a top-corner case per mask kernel, and hub rows over a 2^25-tile span.
   The oracle's dense arrays cannot take that N: the reference is its product on compress_columns' ranks
   (tests/test_compress_columns_host.py holds the helper to the direct product).
D. A call of 2^32 products, and a row of 2^31 (its int32 product count saturates).  Values are integers of
   +-{1, 2, 3}: every sum is exact in any order and the results must equal the reference."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import mhspgemm
from mhspgemm import _lib as L
from oracle import oracle as orc
from _util import (assert_f64_bound, bin_zoo, compress_columns, edge_values, exact_forward, group_zoo, near_zoo, run_zoo,
                   tiny_zoo)
import test_gpu_f64_bound as fb
from test_gpu_f64_bound import FAMILIES, NFT_ENV, fresh_tool, judged_call, reference, values
from test_gpu_nonfinite import CALLS  # FULL_CALLS and perturbed_fem_row_chunked

pytestmark = pytest.mark.gpu

INT_MAX = 2**31 - 1
WIDE_ENV = {"MHS_NO_O32": "1"}


@pytest.fixture(autouse=True)
def _no_switch_from_outside(monkeypatch):
    """The contexts of this file get MHS_NO_O32 from fresh_tool or not at all."""
    monkeypatch.delenv("MHS_NO_O32", raising=False)


def on_device(tool, *mats):
    for X in mats:
        if X.d_ptr is None:
            X.H2D(tool.device)


def judged(t, R, what):
    """judged_call's rules on a reference tuple (A, B, Cp, Ci, exact) of this file."""
    A, B, Cp, Ci, exact = R
    C, tm = mhspgemm.spgemm(t, A, B)
    try:
        p, c, v = C.to_host()
    finally:
        C.release()
    assert np.array_equal(p, Cp), "row_ptr must be bit-exact"
    assert np.array_equal(c, Ci), "col_idx must be bit-exact"
    assert_f64_bound(v, *exact, f"full call, {what}")
    assert tm.nnzC == Cp[-1] and tm.flop == orc.flop(A.col, B.ptr)
    return tm


# --------------------------------------------------- A. the 64-bit-offset twins ---
# numeric bin (mhs_shape.hpp's NumBin) -> the table kernel issue_numeric launches for it
BIN_KERNEL = {1: "k_num_wave_direct<5 KiB>", 2: "k_num_wave_direct<10 KiB>", 3: "k_num_block<256>", 4: "k_num_block<1024>",
              5: "k_num_block<1024, global>", 6: "k_num_wave<grouped, small>", 7: "k_num_wave<grouped, 10 KiB>",
              14: "k_num_wave_hash<5 KiB>", 15: "k_num_wave_hash<10 KiB>"}
TWINS = sorted(BIN_KERNEL.values()) + ["k_copy_hash<4>", "k_copy_hash<8>", "k_copy_hash<16>"]
NUM_WSH = 14


def numeric_kernels(tm, slot_rows):
    """The table kernels the call's numeric plan launched, from its bin counts as plan_numeric decides them
    (mhs_numplan.hpp; tests/numplan_check.cpp holds that function to hand-worked plans).  slot_rows: the call ran
    numeric-first with value slots (MHS_STAT_NFT), so tiny classes 0..3 are copied, by k_copy_hash -- with the lanes
    of the median slot row's class, at most 16 -- where they and the small hash bin are the whole phase."""
    nb = list(tm.num_bins)
    ks, fused = set(), False
    small = nb[8:12]
    if slot_rows and sum(small) > 0:
        fused = nb[NUM_WSH] > 0 and all(nb[b] <= 0 for b in range(1, 16) if b != NUM_WSH and not 8 <= b < 12)
        acc, cmed = 0, 0
        for c in range(4):
            acc += small[c]
            if 2 * acc >= sum(small):
                cmed = c
                break
        if fused:
            ks.add(f"k_copy_hash<{min(16, 4 << cmed)}>")
    for b, kernel in BIN_KERNEL.items():
        if nb[b] > 0 and not (fused and b == NUM_WSH):
            ks.add(kernel)
    return ks


def copy_zoo(median, seed=13):
    """Numeric-first slot rows and small hash rows and nothing else, so the slot copy fuses with the hash bin
    (k_copy_hash).  B: 40 rows of 50 columns scattered over 2 M (a table of 50 tiles: hash mode), 400 rows of two
    columns in [0, 4000).  A: 40 rows that repeat one scattered B row 12 times (600 products, past every tiny
    class; 1680 bytes of tables: the small hash wave bin; no two alike, so no row groups), and slot rows of 2, 8,
    16 and 32 short B rows -- tiny classes 0, 1, 2, 3 by their A entries -- 60 of class `median`, 10 of each
    other: the median slot row is of class `median`, whose lanes (4, 8, 16) the copy takes."""
    rng = np.random.default_rng(seed + median)
    H, T, N = 40, 400, 2_000_000
    brows = [np.unique(rng.integers(0, N, 50)) for _ in range(H)]
    brows += [np.sort(rng.choice(4000, 2, replace=False)) for _ in range(T)]
    Bp = np.zeros(H + T + 1, np.int64)
    Bp[1:] = np.cumsum([len(r) for r in brows])
    Bc = np.concatenate(brows).astype(np.int32)
    arows = [[k] * 12 for k in range(H)]
    for c, na in enumerate((2, 8, 16, 32)):
        for _ in range(60 if c == median else 10):
            arows.append(sorted((H + rng.choice(T, na, replace=False)).tolist()))
    order = rng.permutation(len(arows))
    arows = [arows[i] for i in order]
    Ap = np.zeros(len(arows) + 1, np.int64)
    Ap[1:] = np.cumsum([len(r) for r in arows])
    Ac = np.array([k for r in arows for k in r], np.int32)
    return (len(arows), H + T, Ap.astype(np.int32), Ac), (H + T, N, Bp.astype(np.int32), Bc)


def wave16_zoo():
    """The two 10 KiB wave bins no zoo reaches.  B row k is the full tile k.  A rows 0..7 are 16 consecutive B rows
    each, no two alike: 1024 products and C entries over 16 tiles, 16 * 16 + 1024 * 8 = 8448 bytes of direct
    tables, past the 5 KiB bin and the tiny classes: the 10 KiB direct bin.  Rows 8..10 repeat B row 20 200 times
    and rows 11, 12 B row 21 150 times: two groups of equal rows, small tables, but 12,800 and 9,600 products a
    row, past the 8192 of the small grouped bin: the 10 KiB grouped bin."""
    K = 24
    Bp = 64 * np.arange(K + 1)
    arows = [list(range(j, j + 16)) for j in range(8)] + [[20] * 200] * 3 + [[21] * 150] * 2
    Ap = np.zeros(len(arows) + 1, np.int64)
    Ap[1:] = np.cumsum([len(r) for r in arows])
    Ac = np.array([k for r in arows for k in r], np.int32)
    return (len(arows), K, Ap.astype(np.int32), Ac), (K, 64 * K, Bp.astype(np.int32), np.arange(64 * K, dtype=np.int32))


def wave16_census(t, tm, M):
    assert tm.num_bins[2] == 8 and tm.num_bins[7] == 2, tm.num_bins


@functools.lru_cache(maxsize=None)
def extra_reference(case):
    At, Bt = wave16_zoo() if case == "wave16_zoo" else copy_zoo(COPY_CASES[case])
    A = mhspgemm.CSR(*At, values("wide", len(At[3]), 17))
    B = mhspgemm.CSR(*Bt, values("wide", len(Bt[3]), 1017))
    Cp, Ci, _ = orc.spgemm(A.ptr, A.col, A.val, B.ptr, B.col, B.val, B.N)
    return A, B, Cp, Ci, exact_forward(A, B, Cp, Ci, A.val, B.val)


COPY_CASES = {f"copy_zoo_{lanes}_lanes": median for median, lanes in enumerate((4, 8, 16))}
# the cases this file adds to CALLS: (environment, options, census)
EXTRA_CASES = {case: (NFT_ENV, {L.MHS_OPT_TINY_FIRST_ROWS: 0}, fb.nft_census) for case in COPY_CASES}
EXTRA_CASES["wave16_zoo"] = ({}, {}, wave16_census)
LAUNCHED = {}  # case -> the table kernels its (first) call launched with 64-bit offsets


def wide_case(tool, case, family):
    """One case on a context of its own with MHS_NO_O32=1: the call, judged, and the same call again."""
    if case in EXTRA_CASES:
        R = extra_reference(case)
        env, options, census = EXTRA_CASES[case]
        call = lambda t, what: judged(t, R, f"{case}, {what}")
        A, B = R[:2]
    else:
        name, env, options, census = CALLS[case]
        A, B = reference(name, family)[:2]
        call = lambda t, what: judged_call(t, name, family, f"{case}, {what}")
    on_device(tool, A, B)
    t2 = fresh_tool(tool, {**env, **WIDE_ENV}, options)
    try:
        assert t2.stat("wide_offsets") == 0
        tm = call(t2, "64-bit offsets")
        census(t2, tm, A.M)
        assert t2.stat("wide_offsets") == 1, "the call's plan took the 64-bit offsets"
        kernels = numeric_kernels(tm, t2.stat("nft") == 1)
        print(f"{case}: num_bins {list(tm.num_bins)} nft {t2.stat('nft')} -> {sorted(kernels)}")
        LAUNCHED.setdefault(case, kernels)
        # the same operands again: a speculated hit, but for the numeric-first probe and the row-chunked path
        tm2 = call(t2, "64-bit offsets, the call repeated")
        assert list(tm2.num_bins) == list(tm.num_bins)
        speculates = L.MHS_OPT_TINY_FIRST_ROWS not in options and L.MHS_OPT_MEM_BUDGET not in options
        assert t2.stat("spec") == int(speculates) and t2.stat("spec_miss") == 0, (t2.stat("spec"), t2.stat("spec_miss"))
        assert t2.stat("wide_offsets") == 2, "once per call, speculated or not"
    finally:
        t2.close()
        A.d_release_csr()
        B.d_release_csr()
    return kernels


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("case", list(CALLS))
def test_wide_offsets_full_call(tool, case, family):
    wide_case(tool, case, family)


@pytest.mark.parametrize("case", list(EXTRA_CASES))
def test_wide_offsets_added_case(tool, case):
    kernels = wide_case(tool, case, "wide")
    if case in COPY_CASES:
        assert kernels == {f"k_copy_hash<{case.split('_')[2]}>"}, kernels


def test_counter_stays_zero_without_the_switch(tool):
    A, B = reference("bin_zoo", "narrow")[:2]
    on_device(tool, A, B)
    t2 = fresh_tool(tool, {}, {})
    try:
        for it in range(2):
            judged_call(t2, "bin_zoo", "narrow", f"32-bit offsets, call {it}")
        assert t2.stat("spec") == 1 and t2.stat("wide_offsets") == 0
        assert L.lib().mhs_ctx_stat(t2.ctx, L.MHS_STAT_WIDE_OFFSETS) == 0 and L.lib().mhs_ctx_stat(t2.ctx, 11) == -1
    finally:
        t2.close()
        A.d_release_csr()
        B.d_release_csr()


def test_counter_counts_a_missed_call_once(tool):
    """A pattern change in place under MHS_NO_O32=1: the speculated call misses, its rerun's plan goes out with
    64-bit offsets, and the user call counts once."""
    from test_gpu_spec_duress import assert_c, base_square, oracle_sq, overwrite
    from _util import with_hub_row
    A = base_square()
    A.H2D(tool.device)
    ref1 = oracle_sq(A.ptr, A.col, A.val, A.N)
    p2, c2 = with_hub_row(A.ptr, A.col, A.N, 2000)
    ref2 = oracle_sq(p2, c2, A.val, A.N)
    t2 = fresh_tool(tool, WIDE_ENV, {})
    try:
        for it in range(2):
            C, _ = mhspgemm.spgemm(t2, A, A)
            assert_c(C, ref1, f"call {it}")
        assert (t2.stat("spec"), t2.stat("spec_miss"), t2.stat("wide_offsets")) == (1, 0, 2)
        overwrite(A, p2, c2)
        C, _ = mhspgemm.spgemm(t2, A, A)
        assert_c(C, ref2, "call 2, the pattern changed")
        assert (t2.stat("spec"), t2.stat("spec_miss"), t2.stat("wide_offsets")) == (2, 1, 3)
    finally:
        t2.close()
        A.d_release_csr()


# which case covers which of the twelve 64-bit-offset kernels
COVERED_BY = {
    "k_copy_hash<4>": "copy_zoo_4_lanes",
    "k_copy_hash<8>": "copy_zoo_8_lanes",
    "k_copy_hash<16>": "copy_zoo_16_lanes",
    "k_num_block<1024, global>": "bin_zoo",
    "k_num_block<1024>": "bin_zoo",
    "k_num_block<256>": "bin_zoo",
    "k_num_wave_hash<10 KiB>": "bin_zoo",
    "k_num_wave_hash<5 KiB>": "bin_zoo",
    "k_num_wave_direct<10 KiB>": "wave16_zoo",
    "k_num_wave_direct<5 KiB>": "bin_zoo",
    "k_num_wave<grouped, 10 KiB>": "wave16_zoo",
    "k_num_wave<grouped, small>": "group_zoo",
}


def test_every_twin_ran(tool):
    """Each of the twelve O32 = false instantiations was launched by the case COVERED_BY names for it (cases the
    tests above have not run in this session run here)."""
    assert sorted(COVERED_BY) == sorted(TWINS) and len(TWINS) == 12
    for case in sorted(set(COVERED_BY.values())):
        if case not in LAUNCHED:
            wide_case(tool, case, "wide")
    for kernel, case in COVERED_BY.items():
        assert kernel in LAUNCHED[case], f"{kernel} was not launched by {case}: {sorted(LAUNCHED[case])}"
    print("launched with 64-bit offsets:", {k: COVERED_BY[k] for k in TWINS})


# ------------------------------------------- B. nnz(C) at and one past INT32_MAX ---
ROW0 = 46341           # B row 0 holds this many columns, B row 1 one
AT_LIMIT = (46340, 41707)  # A rows on B row 0, on B row 1: 46340 * 46341 + 41707 = 2^31 - 1 (a prime: no outer product)
ONE_PAST = (46340, 41708)
BUDGET_MIB = 512       # holds the workspace (about 150 MiB) and the numeric-first slots (130 MiB); C would take 25 GB
# A budget below the whole-M workspace, so the call is row-chunked from the start.  For M = 88,048 rows of one entry
# and B's 46,342: the row cache M * 192 * 8 B = 129 MiB, the spill lists 2^20 * 12 B = 12 MiB, the per-row arrays
# about 100 B a row = 8 MiB, B's masks under 1 MiB: about 150 MiB.  Half the rows: 64 + 6 + 4 + 1 = 75 MiB.
CHUNKED_BUDGET_MIB = 100
assert AT_LIMIT[0] * ROW0 + AT_LIMIT[1] == INT_MAX and ONE_PAST[0] * ROW0 + ONE_PAST[1] == INT_MAX + 1


def limit_cols(n0, M):
    """One entry a row: n0 rows on B row 0, spread evenly (every half of the rows stays below the limit), the
    others on B row 1."""
    c = np.ones(M, np.int32)
    c[(np.arange(n0, dtype=np.int64) * M) // n0] = 0
    assert np.count_nonzero(c == 0) == n0
    return c


def limit_pair(n0, n1, first_n0=None):
    """A (M x 2, M = n0 + n1) and B (2 x ROW0) with nnz(A * B) = n0 * ROW0 + n1; first_n0: A starts with that many
    rows on B row 0 instead (a pattern that fits; the full one goes in place later)."""
    M = n0 + n1
    col = limit_cols(n0 if first_n0 is None else first_n0, M)
    A = mhspgemm.CSR(M, 2, np.arange(M + 1, dtype=np.int32), col, edge_values(M, 3))
    Bp = np.array([0, ROW0, ROW0 + 1], np.int32)
    Bc = np.concatenate([np.arange(ROW0), [ROW0 // 2]]).astype(np.int32)
    return A, mhspgemm.CSR(2, ROW0, Bp, Bc, edge_values(ROW0 + 1, 4))


def refused_call(t, A, B):
    """mhs_spgemm on a marked C: (status, message, C was left untouched)."""
    a, b = A.c_view(), B.c_view()
    mark = (-7, -8, -9, 0x1110, 0x2220, 0x3330)
    c = L.mhs_csr(*mark)
    rc = L.lib().mhs_spgemm(t.ctx, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), None)
    msg = L.lib().mhs_last_error(t.ctx).decode()
    return rc, msg, (c.M, c.N, c.nnz, c.ptr, c.col, c.val) == mark


def free_bytes(t):
    t.release()
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info(t.device)[0]


def failure_scenario(tool, n, budget, fail, sync=1):
    """A context under `budget` MiB on which fail(t2, A, B, fit) must end in its error, then: nothing of the
    failed call is kept on the device, and the context multiplies bin_zoo correctly, twice, the second call
    speculated.  Every kernel and stream of the scenario has run once before the free memory is first read (a
    first launch loads code and may grow the queues' scratch)."""
    A, B = limit_pair(*n, first_n0=100)
    full = limit_cols(n[0], A.M)
    zA, zB = reference("bin_zoo", "narrow")[:2]
    on_device(tool, A, B, zA, zB)
    t2 = fresh_tool(tool, {}, {L.MHS_OPT_MEM_BUDGET: BUDGET_MIB, L.MHS_OPT_SYNC: sync})
    try:
        for it in range(2):  # (warm-up: the pattern that fits, plain and speculated ...)
            C, tm = mhspgemm.spgemm(t2, A, B)
            C.release()
            assert tm.nnzC == 100 * ROW0 + A.M - 100
        for it in range(2):  # (... and bin_zoo)
            judged_call(t2, "bin_zoo", "narrow", f"warm-up {it}")
        t2.set_option(L.MHS_OPT_MEM_BUDGET, budget)
        if fail is not speculated_overflow:
            A.d_col.copy_(torch.from_numpy(full))
        before = free_bytes(t2)

        def fit():  # a first call on the pattern that fits, then the full pattern in place
            C, _ = mhspgemm.spgemm(t2, A, B, timing=False)
            C.release()
            torch.cuda.synchronize()  # (MHS_OPT_SYNC 0: the call's kernels still read A)
            A.d_col.copy_(torch.from_numpy(full))
            torch.cuda.synchronize()
        fail(t2, A, B, fit)
        assert free_bytes(t2) == before, "the failed call keeps device memory"
        spec0 = t2.stat("spec")
        for it in range(2):
            judged_call(t2, "bin_zoo", "narrow", f"after the failure, call {it}")
        assert t2.stat("spec") == spec0 + 1, "the second call after the failure speculates"
        assert free_bytes(t2) == before
    finally:
        t2.close()
        for X in (A, B, zA, zB):
            X.d_release_csr()


def limit_is_not_an_overflow(t2, A, B, fit):
    rc, msg, untouched = refused_call(t2, A, B)
    assert (rc, L.STATUS_NAMES[rc]) == (L.MHS_ERR_OOM, "MHS_ERR_OOM"), (rc, msg)
    assert "C itself does not fit" in msg and untouched, msg
    assert t2.stat("spec_miss") == 0


def scan_overflow(t2, A, B, fit):
    rc, msg, untouched = refused_call(t2, A, B)
    assert rc == L.MHS_ERR_OVERFLOW, (rc, msg)
    assert "nnz(C) exceeds INT32_MAX" in msg and "row chunks" not in msg and untouched, msg


def chunked_overflow(t2, A, B, fit):
    rc, msg, untouched = refused_call(t2, A, B)
    assert rc == L.MHS_ERR_OVERFLOW, (rc, msg)
    assert "nnz(C) exceeds INT32_MAX" in msg and "row chunks" in msg and untouched, msg
    assert t2.chunked_calls() == 0


def speculated_overflow(t2, A, B, fit):
    fit()
    spec0, miss0 = t2.stat("spec"), t2.stat("spec_miss")
    rc, msg, untouched = refused_call(t2, A, B)
    assert rc == L.MHS_ERR_OVERFLOW, (rc, msg)
    assert "nnz(C) exceeds INT32_MAX" in msg and untouched, msg
    assert (t2.stat("spec"), t2.stat("spec_miss")) == (spec0 + 1, miss0 + 1), "one miss, and the rerun's verdict"


def test_nnzC_at_int32_max_is_oom_not_overflow(tool):
    """nnz(C) = 2^31 - 1 fits the row pointer: alloc_c refuses its 25 GB under the budget, the call goes row-chunked
    and returns MHS_ERR_OOM right after the counting pass.  MHS_ERR_OVERFLOW here is the bug."""
    failure_scenario(tool, AT_LIMIT, BUDGET_MIB, limit_is_not_an_overflow)


def test_nnzC_one_past_int32_max_overflows_in_scan(tool):
    failure_scenario(tool, ONE_PAST, BUDGET_MIB, scan_overflow)


def test_nnzC_one_past_int32_max_overflows_row_chunked(tool):
    """Row-chunked from the start (the whole-M workspace is past the budget): each chunk's count is below the limit,
    the total after the counting pass is not, and the message says which check spoke."""
    failure_scenario(tool, ONE_PAST, CHUNKED_BUDGET_MIB, chunked_overflow)


@pytest.mark.parametrize("sync", [1, 0])
def test_nnzC_one_past_int32_max_speculated(tool, sync):
    """A call on a pattern that fits, then the overflowing pattern in place: the speculated call misses and its
    rerun returns the overflow."""
    failure_scenario(tool, ONE_PAST, BUDGET_MIB, speculated_overflow, sync=sync)


# ----------------------------------------------------- C. columns up to 2^31 - 2 ---
TOP = INT_MAX - 1  # the last legal column of N = INT32_MAX; its tile is the tile of the INT_MAX sentinel
ZOOS = {"bin_zoo": (bin_zoo, fb.bin_zoo_census), "tiny_zoo": (lambda: tiny_zoo(7), fb.tiny_census),
        "run_zoo": (lambda: run_zoo(5), fb.run_zoo_census), "group_zoo": (lambda: group_zoo(3), fb.group_zoo_census),
        "near_zoo": (near_zoo, fb.near_zoo_census)}
TINY_BINS, TABLE_BINS = range(8, 14), (1, 2, 3, 4, 5, 6, 7, 14, 15)


def top_corner(mask):
    """K = 64, N = INT32_MAX.  B row k ends in a run of columns up to TOP -- the sentinel's tile, its last bit
    included -- after the column TOP - 1000 - k; even rows start with the column k.  The rows' lengths put the
    last entry of a row, the one whose successor is the sentinel, on every kind of lane of the mask kernel:
    `lane` (under 9 entries a row on average: k_mask_lane) has rows of 1..7 entries and of 31, 32 and 33
    (MASK_LANE_LONG = 32: the longer ones go to the whole wave's walk); `group` (k_mask_b<8, 4>: chunks of 8,
    rounds of 32, MASK_LONG * 8 = 128) has rows of 7..9, 15..17, 31..33, 63..65 and 127..130.
    A: rows of 1..40 odd B rows -- confined to the top 1200 columns, a span below 2^23: tiny classes and small
    tables -- rows of 1..40 B rows of both kinds, which span all of N and take tables (a tiny sort key holds 23
    bits of column offset), and one row of all 64."""
    rng = np.random.default_rng(41)
    if mask == "lane":
        lens = [1 + (k + 3) % 7 for k in range(64)]
        for k, ln in zip((9, 10, 21, 22, 33, 34), (31, 31, 32, 32, 33, 33)):
            lens[k] = ln
    else:
        cyc = (7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 130)
        lens = [cyc[k % len(cyc)] for k in range(64)]
    brows = []
    for k, ln in enumerate(lens):
        row, run = [], ln
        if k % 2 == 0 and run >= 2:
            row.append(k)
            run -= 1
        if run >= 2:
            row.append(TOP - 1000 - k)
            run -= 1
        brows.append(np.array(row + list(range(TOP - run + 1, TOP + 1)), np.int64))
    assert all(len(r) == ln and np.all(np.diff(r) > 0) and r[-1] == TOP for r, ln in zip(brows, lens))
    assert brows[0][0] == 0 and all(r[0] > TOP - 1200 for r in brows[1::2])
    avg = sum(lens) // 64
    assert avg < 9 if mask == "lane" else 9 <= avg < 128, avg
    # rows confined to the top: six of at most three short B rows (at most 128 products: tiny classes 0..3) ...
    arows = [np.array(r) for r in ([1], [17], [1, 3], [17, 19], [1, 3, 5], [17, 19, 21])]
    assert max(sum(lens[k] for k in r) for r in arows) <= 128
    odd = np.arange(1, 64, 2)
    for n in range(1, 33):  # ... and of 1..32 of them
        arows.append(np.sort(rng.choice(odd, n, replace=False)))
    for n in range(1, 41):  # rows over all of N: B row 0 (the column 0) and n - 1 others
        arows.append(np.concatenate([[0], np.sort(rng.choice(np.arange(1, 64), n - 1, replace=False))]))
    arows.append(np.arange(64))
    Bp = np.zeros(65, np.int64)
    Bp[1:] = np.cumsum(lens)
    Ap = np.zeros(len(arows) + 1, np.int64)
    Ap[1:] = np.cumsum([len(r) for r in arows])
    return ((len(arows), 64, Ap.astype(np.int32), np.concatenate(arows).astype(np.int32)),
            (64, INT_MAX, Bp.astype(np.int32), np.concatenate(brows).astype(np.int32)))


def hub_rows_wide():
    """tests/test_gpu_parity.py::test_hub_rows_span_rank_and_windows' "wide" case with N = INT32_MAX: six hub rows
    of all 3000 three-entry B rows (about 9 k tiles over a 2^25-tile span: symbolic windows, numeric accumulation
    in C by global atomics) beside 50 small rows."""
    rng = np.random.default_rng(31)
    K = 3000
    brows = [np.unique(rng.integers(0, INT_MAX, 3)) for _ in range(K)]
    brows[0][-1], brows[1][0] = TOP, 0
    Bp = np.zeros(K + 1, np.int64)
    Bp[1:] = np.cumsum([len(r) for r in brows])
    rows = [np.arange(K) for _ in range(6)] + [np.sort(rng.choice(K, 4, replace=False)) for _ in range(50)]
    Ap = np.zeros(len(rows) + 1, np.int64)
    Ap[1:] = np.cumsum([len(r) for r in rows])
    return ((len(rows), K, Ap.astype(np.int32), np.concatenate(rows).astype(np.int32)),
            (K, INT_MAX, Bp.astype(np.int32), np.concatenate(brows).astype(np.int32)))


@functools.lru_cache(maxsize=None)
def big_n_reference(name):
    """(A, B, Cp, Ci, exact) of a case in the N = INT32_MAX column space, with wide values: the oracle's pattern
    and the long-double sums on B's compressed columns, the pattern mapped back to the true columns."""
    if name in ZOOS:
        At, Bt = ZOOS[name][0]()
        K, _, Bp, Bc = Bt[:4]
        shift = (TOP - int(Bc.max())) // 64 * 64  # the largest multiple of 64 that keeps the columns below N
        assert shift % 64 == 0 and int(Bc.max()) + shift <= TOP < int(Bc.max()) + shift + 64
        At, Bt = At[:4], (K, INT_MAX, Bp, (Bc.astype(np.int64) + shift).astype(np.int32))
    else:
        At, Bt = hub_rows_wide() if name == "hub_rows_wide" else top_corner(name.split("_")[-1])
    A = mhspgemm.CSR(*At, values("wide", len(At[3]), 17))
    B = mhspgemm.CSR(*Bt, values("wide", len(Bt[3]), 1017))
    assert B.N == INT_MAX and 0 <= B.col.min() and B.col.max() <= TOP
    ranks, true = compress_columns(B.col)
    Bk = mhspgemm.CSR(B.M, len(true), B.ptr, ranks, B.val)
    Cp, Ck, _ = orc.spgemm(A.ptr, A.col, A.val, Bk.ptr, Bk.col, Bk.val, Bk.N)
    exact = exact_forward(A, Bk, Cp, Ck, A.val, B.val)
    assert exact[1].min(initial=1) >= 1 and exact[1].sum() == orc.flop(A.col, B.ptr)
    return A, B, Cp, true[Ck].astype(np.int32), exact


BIG_N_CASES = list(ZOOS) + ["top_corner_lane", "top_corner_group", "hub_rows_wide"]


@pytest.mark.parametrize("offsets", ["o32", "wide_offsets"])
@pytest.mark.parametrize("name", BIG_N_CASES)
def test_columns_up_to_int32_max(tool, name, offsets):
    R = big_n_reference(name)
    A, B = R[:2]
    on_device(tool, A, B)
    t2 = fresh_tool(tool, WIDE_ENV if offsets == "wide_offsets" else {}, {})
    try:
        tm = judged(t2, R, f"{name}, N = 2^31 - 1, {offsets}")
        print(f"{name}: sym_bins {list(tm.sym_bins)} num_bins {list(tm.num_bins)}")
        assert t2.stat("wide_offsets") == int(offsets == "wide_offsets")
        if name in ZOOS:  # the tiles, the bins and the censuses are those of the unshifted zoo
            ZOOS[name][1](t2, tm, A.M)
        elif name == "hub_rows_wide":
            assert tm.num_bins[4] >= 6, tm.num_bins  # the hub rows run in the 1024-thread kernel
            assert R[3].max() == TOP and R[3].min() == 0
        else:
            assert sum(tm.num_bins[b] for b in TINY_BINS) >= 6, tm.num_bins    # rows confined to the top
            assert sum(tm.num_bins[b] for b in TABLE_BINS) >= 41, tm.num_bins  # rows that span all of N
            assert R[3].max() == TOP and R[3].min() == 0
    finally:
        t2.close()
        A.d_release_csr()
        B.d_release_csr()


# -------------------------------- D. flop counts past 2^32, a row's past 2^31 ---
def exact_call(t, A, B, Cp, Ci, Cv, flop):
    C, tm = mhspgemm.spgemm(t, A, B)
    try:
        p, c, v = C.to_host()
    finally:
        C.release()
    assert tm.flop == flop == orc.flop(A.col, B.ptr), (tm.flop, flop)
    assert tm.nnzC == Cp[-1] == len(Ci)
    assert np.array_equal(p, Cp), "row_ptr must be bit-exact"
    assert np.array_equal(c, Ci), "col_idx must be bit-exact"
    assert np.array_equal(v, Cv), f"{np.count_nonzero(v != Cv)} of {len(Cv)} values differ from the exact product"
    return tm


def test_flop_count_of_2_to_32(tool):
    """A 2048 x 2048, every row full; B 2048 x 5120, every row the same 1024 columns, five apart (80 tiles):
    2^32 products -- the 64-bit sum of the per-block product words is one past 32 bits -- and nnz(C) = 2^21.
    Reference: the dense float64 product, exact on these integers (sums below 9 * 2048)."""
    n, m = 2048, 1024
    bc = 5 * np.arange(m)
    A = mhspgemm.CSR(n, n, n * np.arange(n + 1), np.tile(np.arange(n), n), edge_values(n * n, 1))
    B = mhspgemm.CSR(n, 5 * m, m * np.arange(n + 1), np.tile(bc, n), edge_values(n * m, 2))
    Cv = (A.val.reshape(n, n) @ B.val.reshape(n, m)).reshape(-1)
    assert np.abs(Cv).max() <= 9 * n and np.count_nonzero(Cv) > len(Cv) // 2
    on_device(tool, A, B)
    t2 = fresh_tool(tool, {}, {})
    try:
        tm = exact_call(t2, A, B, (m * np.arange(n + 1)).astype(np.int32), np.tile(bc, n).astype(np.int32), Cv, 2**32)
        print(f"2^32 products: e2e {tm.total_e2e:.2f} ms, numeric {tm.Numeric:.2f} ms, num_bins {list(tm.num_bins)}")
    finally:
        t2.close()
        A.d_release_csr()
        B.d_release_csr()


def test_row_flop_of_2_to_31(tool):
    """A row 0: 2^20 entries, all of column 0 (duplicates are summed); B row 0: 2048 columns, three apart.  The
    row's 2^31 products saturate its int32 count (sat_int) at INT_MAX, which feeds the bins, the group choice and
    the piece walk; the call's count stays 64-bit.  299 ordinary rows follow, none on B row 0, all far below the
    block bins -- so the one row of the block and global bins is row 0.  Reference: the oracle, on A with row 0
    replaced by its one exact equivalent, the entry (0, sum of the row's values)."""
    rng = np.random.default_rng(51)
    K, N, hub, wide = 300, 10_000, 2**20, 2048
    brows = [3 * np.arange(wide)] + [np.unique(rng.integers(0, N, 5)) for _ in range(K - 1)]
    Bp = np.zeros(K + 1, np.int64)
    Bp[1:] = np.cumsum([len(r) for r in brows])
    B = mhspgemm.CSR(K, N, Bp.astype(np.int32), np.concatenate(brows).astype(np.int32), edge_values(int(Bp[-1]), 6))
    rest = [np.sort(rng.choice(np.arange(1, K), int(rng.integers(1, 7)), replace=False)) for _ in range(K - 1)]
    lens = np.array([hub] + [len(r) for r in rest])
    Ap = np.zeros(K + 1, np.int64)
    Ap[1:] = np.cumsum(lens)
    Ac = np.concatenate([np.zeros(hub, np.int64)] + rest).astype(np.int32)
    A = mhspgemm.CSR(K, K, Ap.astype(np.int32), Ac, edge_values(len(Ac), 5))
    s0 = float(A.val[:hub].sum())
    assert s0 != 0.0 and abs(s0) <= 3 * hub
    Ap1 = np.concatenate([[0], Ap[1:] - (hub - 1)]).astype(np.int32)
    Cp, Ci, Cv = orc.spgemm(Ap1, Ac[hub - 1:], np.concatenate([[s0], A.val[hub:]]), B.ptr, B.col, B.val, N)
    assert Cp[1] == wide and np.array_equal(Cv[:wide], s0 * B.val[:wide])
    flop = hub * wide + int(np.diff(Bp)[np.concatenate(rest)].sum())
    assert flop > 2**31 and hub * wide == 2**31
    on_device(tool, A, B)
    t2 = fresh_tool(tool, {}, {})
    try:
        tm = exact_call(t2, A, B, Cp, Ci, Cv, flop)
        print(f"a row of 2^31 products: e2e {tm.total_e2e:.2f} ms, numeric {tm.Numeric:.2f} ms, "
              f"sym_bins {list(tm.sym_bins)} num_bins {list(tm.num_bins)}")
        assert tm.num_bins[3] + tm.num_bins[4] + tm.num_bins[5] == 1, tm.num_bins  # row 0, in a block or global bin
    finally:
        t2.close()
        A.d_release_csr()
        B.d_release_csr()
