"""GPU tests of the kernels in front of the numeric launch (k_mask_b, k_analyze, k_bin_list, k_sym_common, k_scan)
at the places where a change to how they read a row or a block can go wrong: the rounds and chunks a row is read
in and the lane exchanges at their edges, a row's first and last column, the whole-wave path of long rows, group
heads in the block before their members', the rows in front of a block, and bin lists of several bins in one block
("Front kernels": the load schedules this file was written for, and what was kept).

Every case is a full call judged against the oracle: row_ptr and col_idx exactly, the values within the FP64
bound of tests/_util.py (1.01 m 2^-53 S against long-double sums).  Every case runs twice on one context -- the
second call speculates on the first's plan -- and twice on a context whose buffers are poisoned (MHS_POISON, as
tests/test_gpu_poison.py), where the second call gets the first's C back from the pool.  Rows average at least
9 entries in A and in B in every case, so the lane-group kernels run and not the lane-per-row ones.  References
are computed once per case and read only."""
import functools

import numpy as np
import pytest

import mhspgemm
from mhspgemm import synth
from oracle import oracle as orc
from _util import assert_f64_bound, exact_forward, new_values, random_csr
from test_gpu_f64_bound import fresh_tool
from test_gpu_parity import _perturbed_fem

pytestmark = pytest.mark.gpu

# 32-entry rounds (k_analyze, k_mask_b: 8 lanes x 4), 64-entry chunks and 128-entry pairs (the symbolic walk),
# the 128-entry switch to the whole-wave path (AN_LONG, MASK_LONG: 16 x 8), and a row well past it
EDGE_LENGTHS = (0, 1, 8, 9, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 130, 200)
EDGE_M = 2100  # three 1,024-row blocks of k_scan and k_bin_list
EDGE_VARIANTS = ("long_row_first", "long_row_last", "ends_at_nnz")


def rows_of_lengths(lens, N, seed):
    """CSR (ptr, col) with the given row lengths: sorted, distinct columns of [0, N)."""
    rng = np.random.default_rng(seed)
    ptr = np.zeros(len(lens) + 1, np.int64)
    np.cumsum(lens, out=ptr[1:])
    col = np.concatenate([np.sort(rng.choice(N, int(n), replace=False)) for n in lens] + [np.zeros(0, np.int64)])
    return ptr.astype(np.int32), col.astype(np.int32)


def edge_lengths(variant):
    cyc = np.array(EDGE_LENGTHS)
    i = np.arange(EDGE_M)
    if variant == "long_row_first":
        lens = cyc[(i + len(cyc) - 1) % len(cyc)]
        assert lens[0] == 200
    elif variant == "long_row_last":
        lens = cyc[(i + len(cyc) - 1 - (EDGE_M - 1)) % len(cyc)]
        assert lens[-1] == 200
    else:  # the plain cycle: the matrix's last row is not empty, so its last entry is the arrays' last
        lens = cyc[i % len(cyc)]
        assert lens[0] == 0 and lens[-1] == 96
    assert lens.mean() >= 9 and set(lens) == set(EDGE_LENGTHS)
    return lens


def csr(M, N, ptr, col, seed):
    return mhspgemm.CSR(M, N, ptr, col, new_values(len(col), seed, signed=True))


def stencil(n, drop):
    A = synth.fem_grid(n, n, n, 3, seed=n) if drop == 0 else _perturbed_fem(n, n, n, drop, seed=n)
    assert A.M == 3 * n ** 3
    return A, A


def edge_rows_of_a(variant):
    """A with the edge lengths (k_analyze, k_bin_list, the symbolic walk, k_scan) times a B of short rows."""
    K, N = 2400, 6000
    ap, ac = rows_of_lengths(edge_lengths(variant), K, seed=len(variant))
    bp, bc, _ = random_csr(K, N, 10, seed=5)
    return csr(EDGE_M, K, ap, ac, 1), csr(K, N, bp, bc, 2)


def edge_rows_of_b(variant):
    """A of short rows times a B with the edge lengths (k_mask_b: its rounds, carried runs, first and last column)."""
    N = 6000
    ap, ac, _ = random_csr(EDGE_M, EDGE_M, 10, seed=6)
    bp, bc = rows_of_lengths(edge_lengths(variant), N, seed=len(variant) + 50)
    return csr(EDGE_M, EDGE_M, ap, ac, 3), csr(EDGE_M, N, bp, bc, 4)


def scan_edge(M):
    """M rows of about 12 entries (exactly 12 where M is tiny) times a B of about 10 a row."""
    K, N = 64 if M <= 2 else M, 3000
    if M <= 2:
        ap, ac = rows_of_lengths(np.full(M, 12), K, seed=M)
    else:
        ap, ac, _ = random_csr(M, K, 12, seed=M)
    bp, bc, _ = random_csr(K, N, 10, seed=M + 1)
    return csr(M, K, ap, ac, 5), csr(K, N, bp, bc, 6)


def several_bins():
    """Short rows with, in every 1,024-row block, a few rows of 60 and of 300 entries (600 and 3,000 products)."""
    M, K, N = 2100, 2100, 40_000
    lens = np.random.default_rng(8).integers(6, 15, M)
    lens[np.arange(7, M, 97)] = 60
    lens[np.arange(40, M, 331)] = 300
    ap, ac = rows_of_lengths(lens, K, seed=9)
    bp, bc, _ = random_csr(K, N, 10, seed=10)
    return csr(M, K, ap, ac, 7), csr(K, N, bp, bc, 8)


CASES = {
    **{f"a_rows_{v}": functools.partial(edge_rows_of_a, v) for v in EDGE_VARIANTS},
    **{f"b_rows_{v}": functools.partial(edge_rows_of_b, v) for v in EDGE_VARIANTS},
    "dof3_6": functools.partial(stencil, 6, 0),
    "dof3_11": functools.partial(stencil, 11, 0),  # 3,993 rows: groups of three straddle the 1,024-row block edges
    "dof3_6_dropped": functools.partial(stencil, 6, 0.03),
    "dof3_11_dropped": functools.partial(stencil, 11, 0.03),
    "scan_1024_words": functools.partial(scan_edge, 1023),
    "scan_1025_words": functools.partial(scan_edge, 1024),
    "one_row": functools.partial(scan_edge, 1),
    "two_rows": functools.partial(scan_edge, 2),
    "several_bins": several_bins,
}


@functools.lru_cache(maxsize=None)
def reference(case):
    A, B = CASES[case]()
    assert A.nnz >= 9 * A.M and B.nnz >= 9 * B.M, "the lane-group kernels' cases"
    assert np.all(np.diff(A.ptr) >= 0) and A.ptr[-1] == A.nnz == len(A.col)
    Cp, Ci, _ = orc.spgemm(A.ptr, A.col, A.val, B.ptr, B.col, B.val, B.N)
    return A, B, Cp, Ci, exact_forward(A, B, Cp, Ci, A.val, B.val)


def judged(t, case, what):
    A, B, Cp, Ci, exact = reference(case)
    C, tm = mhspgemm.spgemm(t, A, B)
    try:
        p, c, v = C.to_host()
    finally:
        C.release()
    assert np.array_equal(p, Cp), f"{what}: row_ptr must be bit-exact"
    assert np.array_equal(c, Ci), f"{what}: col_idx must be bit-exact"
    assert_f64_bound(v, *exact, f"{case}, {what}")
    assert tm.nnzC == Cp[-1] and tm.flop == exact[1].sum()
    return tm


@pytest.mark.parametrize("case", list(CASES))
def test_front_kernels(tool, case):
    A, B = reference(case)[:2]
    for X in {id(A): A, id(B): B}.values():
        X.H2D(tool.device)
    try:
        for env in ({}, {"MHS_POISON": "255"}):
            t2 = fresh_tool(tool, env, {})
            try:
                for call in (1, 2):
                    tm = judged(t2, case, f"poison {env.get('MHS_POISON')}, call {call}")
                assert (t2.stat("spec"), t2.stat("spec_miss")) == (1, 0), (t2.stat("spec"), t2.stat("spec_miss"))
                assert (t2.stat("poison_fills") > 0) == bool(env)
                if case == "several_bins":
                    print(f"sym_bins {list(tm.sym_bins)} num_bins {list(tm.num_bins)}")
                    assert np.count_nonzero(list(tm.sym_bins)[1:]) >= 2, "k_bin_list reserves for more than one bin"
                    assert np.count_nonzero(list(tm.num_bins)[1:]) >= 2, "k_scan reserves for more than one bin"
            finally:
                t2.close()
    finally:
        A.d_release_csr()
        if B is not A:
            B.d_release_csr()


def test_edge_cases_are_what_they_say():
    """(the matrices, not the GPU) every edge length occurs in each variant; the dof-3 cases have same-pattern
    triples across a 1,024-row block edge; the dropped ones have broken triples."""
    for v in EDGE_VARIANTS:
        lens = edge_lengths(v)
        assert len(lens) == EDGE_M > 2 * 1024
    A = reference("dof3_11")[0]
    rows = [A.col[A.ptr[i]:A.ptr[i + 1]] for i in (1023, 1024, 2046, 2047, 2048, 2049)]
    assert np.array_equal(rows[0], rows[1]) and np.array_equal(rows[3], rows[4]), "a triple on each side of a block edge"
    D = reference("dof3_11_dropped")[0]
    assert D.nnz < A.nnz and np.any(np.diff(D.ptr)[0::3] != np.diff(D.ptr)[1::3])
