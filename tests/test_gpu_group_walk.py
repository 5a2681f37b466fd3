"""GPU tests of the grouped numeric bin's cursor walk (NUM_WSG: k_num_wave<10 KiB, grouped>): a
launch of about the resident set of waves, every wave drawing its row groups from the XCD groups'
row cursors and fetching the next group under the current one's body (csrc/mhs_groupwalk.hpp,
GroupNext in csrc/mhs_kernels.hip).  Every case is compared with the oracle as test_gpu_parity.py
does -- row_ptr and col bit-exact, values to its tolerance -- and checks the NUM_WSG bin's count,
so no case passes through another kernel.

The matrices are dof-3 FEM grids: every node's three rows share one pattern and no two
neighbouring nodes do, so a grid of n nodes is n row groups, all in NUM_WSG."""
import functools

import numpy as np
import pytest

import mhspgemm
from mhspgemm import _lib as L
from mhspgemm import synth
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-6, 1e-12  # (test_gpu_parity.py's)
NUM_WSG = 6               # mhs_shape.hpp's NumBin


@functools.lru_cache(maxsize=None)
def _grid(nx, ny, nz):
    """(A, the oracle's C) of a dof-3 grid, computed once and shared (read-only)."""
    A = synth.fem_grid(nx, ny, nz, 3, seed=5)
    return A, orc.spgemm(A.ptr, A.col, A.val, A.ptr, A.col, A.val, A.N)


def _host_c(C):
    try:
        return C.to_host()
    finally:
        C.release()


def _same_c(ref, got, what=""):
    Cp, Ci, Cv = ref
    p, c, v = got
    assert np.array_equal(p, Cp), f"row_ptr must be bit-exact {what}"
    assert np.array_equal(c, Ci), f"col_idx must be bit-exact {what}"
    assert mhspgemm.compare_tol(Cp, Ci, Cv, p, c, v, RTOL, ATOL)[0], f"values outside 1e-6 relative {what}"


def _run(t, A, ref, groups, what=""):
    C, tm = mhspgemm.spgemm(t, A, A)
    _same_c(ref, _host_c(C), what)
    assert tm.num_bins[NUM_WSG] == groups, (what, tm.num_bins)
    assert tm.nnzC == ref[0][-1]
    return tm


def test_more_groups_than_resident_waves(tool):
    # (a) 9 x 9 x 70 nodes: 17,010 rows, 5,670 groups -- more than the 4,096 waves of 1,024 resident
    # blocks, so the launch is the resident set and some waves draw twice
    A, ref = _grid(9, 9, 70)
    assert A.M == 17010
    A.H2D(tool.device)
    t2 = mhspgemm.Tool(tool.device)
    try:
        _run(t2, A, ref, 5670)
    finally:
        t2.close()


# (b) a launch capped at 8 blocks (32 waves): 325 groups (not a multiple of 8: eighths of 40 and 41)
# make every wave loop about ten times; 27 groups leave waves that draw a "none" at once
@pytest.mark.parametrize("dims, groups", [((5, 5, 13), 325), ((7, 7, 9), 441), ((3, 3, 3), 27)])
def test_capped_grid_waves_loop(tool, dims, groups):
    A, ref = _grid(*dims)
    assert A.M == 3 * groups and groups % 8 != 0
    A.H2D(tool.device)
    t2 = mhspgemm.Tool(tool.device)
    try:
        t2.set_option(L.MHS_OPT_GROUP_GRID, 8)
        _run(t2, A, ref, groups)
        t2.set_option(L.MHS_OPT_GROUP_GRID, 0)  # the derived grid again: a wave a group, static
        _run(t2, A, ref, groups)
    finally:
        t2.close()


@pytest.mark.parametrize("dims, groups, cap", [((9, 9, 70), 5670, 0), ((5, 5, 13), 325, 8)])
def test_speculated_calls_and_miss(tool, dims, groups, cap):
    # (c) three calls on the same arrays: the second and third queue the first's plan behind the
    # scan, each on freshly zeroed cursors; then a new pattern in the same arrays: the scan rejects
    # the plan, its grouped launch returns before it draws a ticket, the call reruns
    import torch
    A0, ref = _grid(*dims)
    A = mhspgemm.CSR(A0.M, A0.N, A0.ptr.copy(), A0.col.copy(), A0.val.copy())
    A.H2D(tool.device)
    t2 = mhspgemm.Tool(tool.device)
    try:
        if cap:
            t2.set_option(L.MHS_OPT_GROUP_GRID, cap)
        for it in range(3):
            _run(t2, A, ref, groups, f"call {it}")
        assert t2.stat("spec") == 2 and t2.stat("spec_miss") == 0, (t2.stat("spec"), t2.stat("spec_miss"))
        # the rows of the first 40 nodes take new columns (same row lengths): 40 groups dissolve
        rng = np.random.default_rng(3)
        col2 = A0.col.copy()
        for r in range(120):
            a0, a1 = int(A0.ptr[r]), int(A0.ptr[r + 1])
            col2[a0:a1] = np.sort(rng.choice(A0.N, a1 - a0, replace=False)).astype(np.int32)
        A.d_col.copy_(torch.from_numpy(col2))
        ref2 = orc.spgemm(A0.ptr, col2, A0.val, A0.ptr, col2, A0.val, A0.N)
        C, tm = mhspgemm.spgemm(t2, A, A)
        _same_c(ref2, _host_c(C), "after the pattern change")
        assert t2.stat("spec") == 3 and t2.stat("spec_miss") == 1, (t2.stat("spec"), t2.stat("spec_miss"))
        assert 0 < tm.num_bins[NUM_WSG] < groups, tm.num_bins
        kept = tm.num_bins[NUM_WSG]
        C, tm = mhspgemm.spgemm(t2, A, A)  # the rerun left its own plan: a hit
        _same_c(ref2, _host_c(C), "the call after the rerun")
        assert t2.stat("spec") == 4 and t2.stat("spec_miss") == 1 and tm.num_bins[NUM_WSG] == kept
    finally:
        t2.close()
        A.d_release_csr()


def test_row_chunked_launches(tool, monkeypatch):
    # (d) the 325-group grid row-chunked: a row cache of 2,000 tiles a row (24 KB: 23 MB for the 975
    # rows) does not fit a 20 MiB budget, half the rows' does -- two chunks, each with a front pass
    # that zeroes the cursors and a capped grouped launch of its own.  The chunk boundary (488 rows)
    # cuts node 162 into a group of two rows and a single row, and in the second chunk, whose nodes
    # start at rows 1 + 3k, every run break (a multiple of 96 rows) does the same to one more node,
    # five in all: 163 + 162 groups, six rows on their own in the small wave bin.
    monkeypatch.setenv("MHS_MC_LIST", "2000")
    monkeypatch.setenv("MHS_SPILL_CAP", "65536")
    A, ref = _grid(5, 5, 13)
    A.H2D(tool.device)
    t2 = mhspgemm.Tool(tool.device)
    try:
        t2.set_option(L.MHS_OPT_GROUP_GRID, 8)
        t2.set_option(L.MHS_OPT_MEM_BUDGET, 20)
        C, tm = mhspgemm.spgemm(t2, A, A)
        _same_c(ref, _host_c(C))
        assert t2.chunked_calls() == 1
        assert tm.num_bins[NUM_WSG] == 325 and tm.num_bins[1] == 6, tm.num_bins
    finally:
        t2.close()
