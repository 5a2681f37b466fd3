"""Speculated calls under duress: the rows of spec_outcome's table (csrc/mhs_shape.hpp) that the
speculation tests of test_gpu_parity.py do not reach -- no room for the plan's C (MHS_SPEC_NO_ROOM) with the
pattern unchanged and changed in place, a miss whose left-out rows hold stale offsets that overflow k_scan's sum,
a miss whose rerun goes row-chunked, a genuine input error written under a valid plan, and the counters of a
missed call.  tests/spec_outcome_check.cpp shows on the host which rows the earlier expression got wrong.

A speculated call leaves out the k_sym_rare / k_sym_block<256> launches whose bins its plan had empty; a row of
the new contents that falls in such a bin keeps what its C.ptr slot held (the pool's last row pointer).  The row
shape used for that here: more than SYM_WAVE_WORK tile products with a table that fits the 256-thread block bin
(sym_bin_of: SYM_B256; the symwork_wave_b256 rung of tests/golden/shape_edges.json), past the tiny classes'
512 products.

Every C is compared with the oracle's for the pattern then in the device arrays: row pointer and columns
bit-exact, values within RTOL / ATOL."""
import numpy as np
import pytest

import mhspgemm
from mhspgemm import synth
from oracle import oracle as orc
from _util import ATOL, RTOL, load_edges, random_csr, row_shapes, with_hub_row

pytestmark = pytest.mark.gpu

SYM_B256, SYM_B1024, SYM_GLOBAL, SYM_WM = 2, 3, 4, 11  # mhs_shape.hpp SymBin (timing.sym_bins)
SYM_WAVE_WORK = load_edges()["constants"]["SYM_WAVE_WORK"]
TINY_FLOP_MAX = 512  # the largest symbolic sort class (64 lanes x 8)
M0 = 4096


def oracle_sq(p, c, v, N):
    return orc.spgemm(p, c, v, p, c, v, N)


def assert_c(C, ref, what=""):
    """C (released to its context) is the oracle's `ref`."""
    try:
        p, c, v = C.to_host()
    finally:
        C.release()
    Cp, Ci, Cv = ref
    assert np.array_equal(p, Cp) and np.array_equal(c, Ci), f"pattern {what}"
    ok, _, _, bv, mr = mhspgemm.compare_tol(Cp, Ci, Cv, p, c, v, RTOL, ATOL)
    assert ok, f"{bv} values outside 1e-6 relative (max {mr:.3e}) {what}"


def rare_rows(t):
    return t.sym_bins[SYM_WM] + t.sym_bins[SYM_B1024] + t.sym_bins[SYM_GLOBAL]


def overwrite(A, ptr=None, col=None):
    """New contents in A's device arrays (same sizes, same addresses)."""
    import torch
    if ptr is not None:
        assert len(ptr) == A.d_ptr.numel()
        A.d_ptr.copy_(torch.from_numpy(np.ascontiguousarray(ptr, np.int32)))
    if col is not None:
        assert len(col) == A.d_col.numel()
        A.d_col.copy_(torch.from_numpy(np.ascontiguousarray(col, np.int32)))
    torch.cuda.synchronize()


def base_square(seed=21):
    p, c, v = random_csr(M0, M0, 8, seed=seed)
    return mhspgemm.CSR(M0, M0, p, c, v)


def hub_is_left_out(p2, c2, v, ref2, N):
    """Row 0 of the changed pattern lands in SYM_B256, a bin the base matrix leaves empty."""
    A2 = (len(p2) - 1, N, p2, c2, v)
    sh = row_shapes(A2, A2, ref2[0], ref2[1])
    return sh["tflop"][0] > SYM_WAVE_WORK and sh["flop"][0] > TINY_FLOP_MAX and sh["tflop"][0] <= (1 << 20)


def call_reusing_ptr(tool, A, B, last_ptr, timing=False):
    """One call whose C.ptr must be the buffer the previous C gave back: the pooled row pointer, whose contents a
    left-out row keeps."""
    C, t = mhspgemm.spgemm(tool, A, B, timing=timing)
    if last_ptr is not None:
        assert C.c.ptr == last_ptr, "the released row pointer was not reused: the test's precondition"
    return C, t, C.c.ptr


def test_no_room_same_pattern(tool, monkeypatch):
    """(spec, !launched, !err, same): the plan's C does not fit, nothing changed -- the call goes on from its own
    Stats (they are the plan's: what the trimmed symbolic pass left out was empty) and must not rerun."""
    monkeypatch.setenv("MHS_SPEC_NO_ROOM", "1")
    A = base_square()
    A.H2D(tool.device)
    ref = oracle_sq(A.ptr, A.col, A.val, A.N)
    t2 = mhspgemm.Tool(tool.device)
    try:
        for it in range(3):
            C, t = mhspgemm.spgemm(t2, A, A, timing=(it == 1))
            if t is not None:
                assert t.nnzC == ref[0][-1] and t.flop == orc.flop(A.col, A.ptr)
                assert rare_rows(t) == 0 and t.sym_bins[SYM_B256] == 0, t.sym_bins  # both launches are left out
            assert_c(C, ref, f"call {it}")
        # calls 1 and 2 speculated (each left out two symbolic launches), but phase A never went out
        assert t2.stat("spec_skipped") == 4
        assert t2.stat("spec") == 0 and t2.stat("spec_miss") == 0 and t2.chunked_calls() == 0
    finally:
        t2.close()
        A.d_release_csr()


def test_no_room_pattern_changed(tool, monkeypatch):
    """ADVICE r6 (high).  (spec, !launched, !err, !same): the plan's C does not fit and the pattern changed in
    place into a left-out bin -- the call's Stats hold the hub row's stale count, so C must not be built from
    them: a rerun.  (The rerun was keyed on `launched`: C was sized and filled from the stale scan.)"""
    monkeypatch.setenv("MHS_SPEC_NO_ROOM", "1")
    A = base_square()
    A.H2D(tool.device)
    ref1 = oracle_sq(A.ptr, A.col, A.val, A.N)
    p2, c2 = with_hub_row(A.ptr, A.col, A.N, 2000)
    ref2 = oracle_sq(p2, c2, A.val, A.N)
    assert hub_is_left_out(p2, c2, A.val, ref2, A.N)
    t2 = mhspgemm.Tool(tool.device)
    try:
        C, t, last = call_reusing_ptr(t2, A, A, None, timing=True)
        assert rare_rows(t) == 0 and t.sym_bins[SYM_B256] == 0, t.sym_bins
        assert_c(C, ref1, "call 0")
        C, _, last = call_reusing_ptr(t2, A, A, last)
        assert_c(C, ref1, "call 1")
        assert t2.stat("spec_skipped") == 2 and t2.stat("spec_miss") == 0
        overwrite(A, p2, c2)
        C, t, last = call_reusing_ptr(t2, A, A, last, timing=True)
        assert t.sym_bins[SYM_B256] >= 1, t.sym_bins  # (the rerun's Stats: the hub row was counted)
        assert_c(C, ref2, "call 2, the pattern changed")
        assert t2.stat("spec_miss") == 1 and t2.stat("spec_skipped") == 4
        C, _, last = call_reusing_ptr(t2, A, A, last)
        assert_c(C, ref2, "call 3")
        assert t2.stat("spec_miss") == 1 and t2.stat("spec") == 0 and t2.chunked_calls() == 0
    finally:
        t2.close()
        A.d_release_csr()


def overflow_pair():
    """A (8192 x 1104) in two patterns of one size and B (1104 x 65536).  B rows 0..1023 hold the 64 columns of
    tile k; rows 1024..1103 one column in each of the tiles 0..63.  Pattern 1: every A row is 16 consecutive
    narrow B rows (1024 products over 16 tiles: the wave bin; starts 37 rows apart, so no two neighbours share a
    first column) -- C has 8192 * 1024 = 8 388 608 entries and row pointer entries of about 8e6 at its last rows.
    Pattern 2: the last 400 rows are 65 wide B rows each (65 * 64 = 4160 tile products > SYM_WAVE_WORK, a
    64-tile table: SYM_B256), paid for by emptying the 1225 rows in front of them (400 * (65 - 16) = 1225 * 16)."""
    M, KN, KW, per, hubs, wide = 8192, 1024, 80, 16, 400, 65
    K, N = KN + KW, 64 * KN
    assert wide * 64 > SYM_WAVE_WORK and wide * 64 > TINY_FLOP_MAX
    blen = np.full(K, 64)
    bcol = np.concatenate([64 * np.repeat(np.arange(KN), 64) + np.tile(np.arange(64), KN),
                           np.tile(64 * np.arange(64), KW) + np.repeat(np.arange(KW) % 64, 64)]).astype(np.int32)
    Bp = np.zeros(K + 1, np.int64)
    np.cumsum(blen, out=Bp[1:])
    start = (37 * np.arange(M)) % (KN - per)
    c1 = (start[:, None] + np.arange(per)[None, :]).reshape(-1).astype(np.int32)
    p1 = (per * np.arange(M + 1)).astype(np.int32)
    emptied = hubs * (wide - per) // per
    assert hubs * (wide - per) == emptied * per
    len2 = np.full(M, per)
    len2[M - hubs - emptied:M - hubs] = 0
    len2[M - hubs:] = wide
    p2 = np.zeros(M + 1, np.int64)
    np.cumsum(len2, out=p2[1:])
    keep = M - hubs - emptied
    hub_cols = KN + (np.arange(hubs)[:, None] % (KW - wide + 1)) + np.arange(wide)[None, :]
    c2 = np.concatenate([c1[:keep * per], hub_cols.reshape(-1)]).astype(np.int32)
    assert len(c2) == len(c1) and p2[-1] == p1[-1]
    rng = np.random.default_rng(31)
    av, bv = rng.uniform(0.1, 1.0, len(c1)), rng.uniform(0.1, 1.0, len(bcol))
    return (M, K, N, hubs), (p1, c1, av), (p2.astype(np.int32), c2, av), (Bp.astype(np.int32), bcol, bv)


def test_miss_with_false_overflow(tool):
    """ADVICE r6 (medium).  (spec, launched, err, !same): 400 rows of the changed pattern fall in the left-out
    SYM_B256 bin and keep the previous row pointer's entries, about 8e6 each; k_scan's sum of them passes
    INT32_MAX and sets the overflow bit for a product of 8.4e6 entries.  The error bit of a speculated call is not
    the call's result: the call reruns and returns the oracle's C.  (A miss with an error bit did not rerun: this
    call failed with MHS_ERR_OVERFLOW, "nnz(C) exceeds INT32_MAX".)"""
    (M, K, N, hubs), (p1, c1, av), (p2, c2, _), (Bp, Bc, bv) = overflow_pair()
    A = mhspgemm.CSR(M, K, p1, c1, av)
    B = mhspgemm.CSR(K, N, Bp, Bc, bv)
    A.H2D(tool.device)
    B.H2D(tool.device)
    ref1 = orc.spgemm(p1, c1, av, Bp, Bc, bv, N)
    ref2 = orc.spgemm(p2, c2, av, Bp, Bc, bv, N)
    assert orc.flop(c1, Bp) < 5e7 and orc.flop(c2, Bp) < 5e7
    t2 = mhspgemm.Tool(tool.device)
    try:
        C, t, last = call_reusing_ptr(t2, A, B, None, timing=True)
        assert rare_rows(t) == 0 and t.sym_bins[SYM_B256] == 0, t.sym_bins
        first_ptr = C.to_host()[0]
        assert_c(C, ref1, "call 0")
        C, _, last = call_reusing_ptr(t2, A, B, last)
        assert_c(C, ref1, "call 1")
        assert t2.stat("spec") == 1 and t2.stat("spec_skipped") == 2 and t2.stat("spec_miss") == 0
        # not vacuous: the stale entries alone pass INT32_MAX, the product itself is far below it
        stale = int(first_ptr[M - hubs:M].astype(np.int64).sum())
        assert stale > np.iinfo(np.int32).max and int(ref2[0][-1]) < (1 << 24), (stale, int(ref2[0][-1]))
        overwrite(A, p2, c2)
        C, t, last = call_reusing_ptr(t2, A, B, last, timing=True)
        assert t.sym_bins[SYM_B256] == hubs, t.sym_bins
        assert_c(C, ref2, "call 2, the pattern changed")
        assert t2.stat("spec") == 2 and t2.stat("spec_miss") == 1 and t2.stat("spec_skipped") == 4
        C, _, last = call_reusing_ptr(t2, A, B, last)
        assert_c(C, ref2, "call 3")
        assert t2.stat("spec") == 3 and t2.stat("spec_miss") == 1  # the rerun's own plan: a hit
    finally:
        t2.close()
        A.d_release_csr()
        B.d_release_csr()


def test_miss_then_chunked(tool):
    """A miss whose rerun finds no room for its own C beside the workspace: the second attempt goes row-chunked.
    The changed pattern has the hub row and 1100 rows that take its columns in A*A."""
    from mhspgemm import _lib as L
    A = base_square()
    A.H2D(tool.device)
    ref1 = oracle_sq(A.ptr, A.col, A.val, A.N)
    p2, c2 = with_hub_row(A.ptr, A.col, A.N, 2000, feed=1100)
    ref2 = oracle_sq(p2, c2, A.val, A.N)
    assert hub_is_left_out(p2, c2, A.val, ref2, A.N)
    # The budget, 40 MiB, against what the context holds for 4096 rows and 32 K entries: the workspace is about
    # 21 MiB (row cache 4096 * 1536 B = 6 MiB, spill lists 2^20 * 12 B = 12 MiB, B's masks, bin lists and the
    # near-group rows about 3 MiB; 23 MiB with the 1/8 head room), the numeric-first slots 4096 * 128 * 12 B =
    # 6 MiB (under 7 with head room): at most 30 MiB held.  The first pattern's C, about 2.5e5 entries * 12 B =
    # 3 MiB, fits beside that (33 <= 40); the changed pattern's, over 2.2e6 entries = more than 25 MiB, does not
    # (21 + 25 > 40) but fits alone (under 30 MiB <= 40) and beside a 2048-row workspace (about 10 MiB).
    n1, n2 = int(ref1[0][-1]), int(ref2[0][-1])
    assert n1 * 12 <= 4 << 20 and (25 << 20) <= n2 * 12 <= (30 << 20), (n1, n2)
    t2 = mhspgemm.Tool(tool.device)
    try:
        t2.set_option(L.MHS_OPT_MEM_BUDGET, 40)
        for it in range(2):
            C, _ = mhspgemm.spgemm(t2, A, A, timing=False)
            assert_c(C, ref1, f"call {it}")
        assert t2.stat("spec") == 1 and t2.stat("spec_miss") == 0 and t2.chunked_calls() == 0
        overwrite(A, p2, c2)
        C, t = mhspgemm.spgemm(t2, A, A)
        assert t.nnzC == n2 and t.flop == orc.flop(c2, p2)
        assert_c(C, ref2, "call 2, the pattern changed")
        assert t2.stat("spec") == 2 and t2.stat("spec_miss") == 1 and t2.chunked_calls() == 1
    finally:
        t2.close()
        A.d_release_csr()


def test_genuine_error_in_place(tool):
    """(spec, launched, err): two columns of one row of B swapped under a valid plan.  The speculated call does
    not trust its error bit, the rerun finds the error again and reports it; the failed call leaves no plan, so
    the next call does not speculate and the one after it does.  Synchronised and unsynchronised calls alike."""
    from mhspgemm import _lib as L
    A = base_square()
    A.H2D(tool.device)
    ref = oracle_sq(A.ptr, A.col, A.val, A.N)
    r = int(np.argmax(np.diff(A.ptr) >= 2))
    bad = A.col.copy()
    i = int(A.ptr[r])
    bad[i], bad[i + 1] = A.col[i + 1], A.col[i]
    assert bad[i] > bad[i + 1]
    t2 = mhspgemm.Tool(tool.device)
    try:
        misses = 0
        for sync in (1, 0):
            t2.set_option(L.MHS_OPT_SYNC, sync)
            for it in range(2):  # a valid plan (set by the first call, or left by the round before)
                C, _ = mhspgemm.spgemm(t2, A, A, timing=False)
                assert_c(C, ref, f"sync {sync} call {it}")
            spec0 = t2.stat("spec")
            overwrite(A, col=bad)
            with pytest.raises(mhspgemm.MHSpGEMMError) as e:
                mhspgemm.spgemm(t2, A, A, timing=False)
            assert e.value.status == 3 and "not sorted" in str(e.value), str(e.value)
            misses += 1
            assert t2.stat("spec_miss") == misses
            overwrite(A, col=A.col)
            spec1 = t2.stat("spec")
            assert spec1 <= spec0 + 1
            C, _ = mhspgemm.spgemm(t2, A, A, timing=False)
            assert_c(C, ref, f"sync {sync}, restored")
            assert t2.stat("spec") == spec1, "the failed call left no plan"
            C, _ = mhspgemm.spgemm(t2, A, A, timing=False)
            assert_c(C, ref, f"sync {sync}, restored, second call")
            assert t2.stat("spec") == spec1 + 1 and t2.stat("spec_miss") == misses
    finally:
        t2.close()
        A.d_release_csr()


@pytest.mark.parametrize("mode", ["default", "forked"])
def test_counters_once_per_call(tool, mode, monkeypatch):
    """ADVICE r6 (low).  MHS_STAT_SYM_FORK and MHS_STAT_SPEC_SKIPPED count user calls: the second attempt of a
    missed call adds nothing.  By launch_symbolic's rules on scircuit-like, whose plan has rows in the rare symbolic bins:
    default -- the first call does not fork (fewer than 2^19 rows, no probe), a speculated attempt forks its
    plan's rare rows, the rerun does not: sym_fork 0, 1, 2 (the miss: one, not two attempts counted), 3;
    forked (MHS_SYM_FORK=1, MHS_SPEC_FORK=1) -- every attempt forks: sym_fork 1, 2, 3 (the miss; two attempts
    forked), 4.  A forked pass leaves no launch out: spec_skipped stays 0."""
    if mode == "forked":
        monkeypatch.setenv("MHS_SYM_FORK", "1")
        monkeypatch.setenv("MHS_SPEC_FORK", "1")
    A = synth.SYNTH["scircuit"]()
    A.H2D(tool.device)
    rng = np.random.default_rng(11)
    c2 = A.col.copy()
    for r in range(0, A.M, 7):  # every 7th row's columns redrawn (same length, sorted)
        a0, a1 = int(A.ptr[r]), int(A.ptr[r + 1])
        if a1 > a0:
            c2[a0:a1] = np.sort(rng.choice(A.N, a1 - a0, replace=False)).astype(np.int32)
    ref1 = oracle_sq(A.ptr, A.col, A.val, A.N)
    ref2 = oracle_sq(A.ptr, c2, A.val, A.N)
    base = 1 if mode == "forked" else 0
    t2 = mhspgemm.Tool(tool.device)
    try:
        C, t = mhspgemm.spgemm(t2, A, A)
        assert rare_rows(t) > 0, t.sym_bins
        assert_c(C, ref1, "call 0")
        assert t2.stat("sym_fork") == base
        C, _ = mhspgemm.spgemm(t2, A, A, timing=False)
        assert_c(C, ref1, "call 1")
        assert t2.stat("spec") == 1 and t2.stat("sym_fork") == base + 1 and t2.stat("spec_miss") == 0
        overwrite(A, col=c2)
        C, t = mhspgemm.spgemm(t2, A, A)
        assert rare_rows(t) > 0, t.sym_bins  # (the next call's plan forks too)
        assert_c(C, ref2, "call 2, the pattern changed")
        assert t2.stat("spec") == 2 and t2.stat("spec_miss") == 1
        assert t2.stat("sym_fork") == base + 2, t2.stat("sym_fork")
        C, _ = mhspgemm.spgemm(t2, A, A, timing=False)
        assert_c(C, ref2, "call 3")
        assert t2.stat("spec") == 3 and t2.stat("spec_miss") == 1 and t2.stat("sym_fork") == base + 3
        assert t2.stat("spec_skipped") == 0
    finally:
        t2.close()
        A.d_release_csr()
