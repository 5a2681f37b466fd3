"""GPU tests of the full call (mhs_spgemm) on operands whose B rows repeat column indices.

include/mhspgemm.h takes B rows that ascend, not strictly, and promises sums over every stored entry.  The inputs
are the repeat twins of tests/_dups.py -- the suite's zoos and FEM grids with repeats placed at the row's ends,
across the chunk edges of the mask formation, on both sides of a tile edge, one column 65 and 200 times, rows
doubled, adjacent rows with one pattern and equal or different multiplicities -- and they run on every numeric
path a context can be switched to: every entry of tests/test_gpu_f64_bound.py's FULL_CALLS on the twin of its
operands, with the entry's census unchanged, plus 64-bit offsets, the slot copy (k_copy_hash) and the 10 KiB wave
bins, a speculated second call, A * A on matrices that hold repeats themselves (near groups and union runs), and
a case per mask-formation kernel.  Values are integers
of +-{1, 2, 3}, so every sum is exact in any order: row_ptr, col_idx and the values must equal the oracle's
(np.array_equal; no tolerance anywhere), and nnzC and flop its counts.  tests/test_b_repeats_host.py holds the
oracle on a twin to the oracle on the merged twin, without a GPU."""
import functools

import numpy as np
import pytest

import mhspgemm
from oracle import oracle as orc
from _dups import ALIASED, KINDS, UNIFORM, present, twin_operands, with_repeats
from _util import edge_values, expand
from test_gpu_f64_bound import FULL_CALLS, fresh_tool
import test_gpu_scale_edges as se
from test_gpu_scale_edges import WIDE_ENV, on_device

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _no_switch_from_outside(monkeypatch):
    monkeypatch.delenv("MHS_NO_O32", raising=False)


def exact_reference(At, Bt):
    """(A, B, Cp, Ci, Cv) of operand tuples with integer values (Bt None: B is A), after the host-side assert that
    the sums are exact."""
    A = mhspgemm.CSR(*At)
    B = A if Bt is None else mhspgemm.CSR(*Bt)
    Cp, Ci, Cv = orc.spgemm(A.ptr, A.col, A.val, B.ptr, B.col, B.val, B.N)
    _, _, s = expand(A.ptr, A.col, B.ptr, B.col, Cp, Ci, B.N)
    assert len(s) == orc.flop(A.col, B.ptr) and 9 * int(np.bincount(s).max()) < 2 ** 24, "integers below 2^24: exact"
    return A, B, Cp, Ci, Cv


@functools.lru_cache(maxsize=None)
def reference(name):
    """The twin of a case of _dups.twin_operands, its exact product and the counts of its repeat kinds.  Read only."""
    At, Bt, counts, _ = twin_operands(name)
    return (*exact_reference(At, Bt), counts)


def judged_exact(t, R, what):
    A, B, Cp, Ci, Cv = R[:5]
    C, tm = mhspgemm.spgemm(t, A, B)
    try:
        p, c, v = C.to_host()
    finally:
        C.release()
    assert np.array_equal(p, Cp), f"{what}: row_ptr must be bit-exact"
    assert np.array_equal(c, Ci), f"{what}: col_idx must be bit-exact"
    assert np.array_equal(v, Cv), f"{what}: {np.count_nonzero(v != Cv)} of {len(Cv)} values differ from the exact product"
    assert tm.nnzC == Cp[-1] and tm.flop == orc.flop(A.col, B.ptr), what
    return tm


def kinds_for(name):
    """The kinds a case's twin must hold (tests/test_b_repeats_host.py says why the others cannot be there)."""
    if name in UNIFORM:
        return set("abcdgi")
    return set("abcdefi") if name in ("bin_zoo", "tiny_zoo") else set(KINDS)


def run_case(tool, name, env, options, census, what):
    R = reference(name)
    A, B, counts = R[0], R[1], R[5]
    assert present(counts) >= kinds_for(name), counts
    on_device(tool, A, B)
    t2 = fresh_tool(tool, env, options)
    try:
        tm = judged_exact(t2, R, what)
        print(f"{what}: sym_bins {list(tm.sym_bins)} num_bins {list(tm.num_bins)} near {t2.stat('near')} nft {t2.stat('nft')}")
        census(t2, tm, A.M)
        return t2.stat("near"), t2.stat("wide_offsets")
    finally:
        t2.close()
        A.d_release_csr()
        B.d_release_csr()


# ------------------------------------------------------------------ every entry of FULL_CALLS, on its twin ---
@pytest.mark.parametrize("case", list(FULL_CALLS))
def test_repeats_full_call(tool, case):
    """The entry's context and census on the repeat twin of its operands.  The FEM entries multiply A by itself, so
    the twin is A: the uniform variant of _dups.ALIASED, in which the dof rows of a node stay identical and the
    capped grid's 325 row groups stay 325; perturbed_fem takes the ragged variant."""
    name, env, options, census = FULL_CALLS[case]
    run_case(tool, name, env, options, census, case)


# ------------------------------------------------------------------ A * A on a matrix with repeats ---
@pytest.mark.parametrize("name", list(ALIASED))
def test_repeats_aliased_square(tool, name):
    """A * A with B being A (B's near groups walk union rows built from rows that hold repeats), then the same
    product with B an unaliased copy (no union runs).  Ragged variants: near groups were verified."""
    R = reference(name)
    A, counts = R[0], R[5]
    assert R[1] is A and present(counts) >= kinds_for(name), counts
    on_device(tool, A)
    Bc = mhspgemm.CSR(A.M, A.N, A.ptr.copy(), A.col.copy(), A.val.copy())
    Bc.H2D(tool.device)
    t2 = fresh_tool(tool, {}, {})
    try:
        tm = judged_exact(t2, R, f"{name}, B is A")
        print(f"{name}: num_bins {list(tm.num_bins)} near {t2.stat('near')}")
        assert tm.num_bins[6] + tm.num_bins[7] > 0, tm.num_bins
        if name not in UNIFORM:
            assert t2.stat("near") >= 1, "near groups were verified: union rows were built from rows with repeats"
        judged_exact(t2, (A, Bc) + R[2:], f"{name}, B an unaliased copy")
    finally:
        t2.close()
        A.d_release_csr()
        Bc.d_release_csr()


# ------------------------------------------------------------------ 64-bit offsets ---
@pytest.mark.parametrize("case", ["bin_zoo", "tiny_zoo"])
def test_repeats_wide_offsets(tool, case):
    name, env, options, census = FULL_CALLS[case]
    near, wide = run_case(tool, name, {**env, **WIDE_ENV}, options, census, f"{case}, 64-bit offsets")
    assert wide == 1, "the call's plan took the 64-bit offsets"


# ------------------------------------------------------------------ the slot copy and the 10 KiB wave bins ---
@functools.lru_cache(maxsize=None)
def added_reference(case):
    """tests/test_gpu_scale_edges.py's inputs for the kernels no zoo reaches, B with repeats.  Kind e and the inflated
    c stay out: a row of 65 or 200 more entries takes its A rows out of the tiny classes (copy_zoo: the slot copy
    then no longer fuses with the small hash bin) or past the 32,768 products of the 10 KiB wave bins (wave16_zoo)."""
    At, Bt = se.wave16_zoo() if case == "wave16_zoo" else se.copy_zoo(se.COPY_CASES[case])
    twin, counts = with_repeats((*Bt, np.zeros(len(Bt[3]))), 9, share=0.05, kinds="abcdfghi", inflate=False)
    return (*exact_reference((*At, edge_values(len(At[3]), 10)), twin), counts)


@pytest.mark.parametrize("case", list(se.EXTRA_CASES))
def test_repeats_added_case(tool, case):
    """copy_zoo: numeric-first slot rows copied by k_copy_hash with 4, 8 and 16 lanes, fused with the small hash bin;
    wave16_zoo: the 10 KiB direct and grouped wave bins.  The censuses and the launched kernels are those of the
    clean inputs."""
    R = added_reference(case)
    A, B, counts = R[0], R[1], R[5]
    # (wave16_zoo's B rows are one tile each: no tile edge inside a row, so no kind d; neither B has adjacent equal rows)
    assert present(counts) >= (set("abfi") if case == "wave16_zoo" else set("abdfi")), counts
    env, options, census = se.EXTRA_CASES[case]
    on_device(tool, A, B)
    t2 = fresh_tool(tool, env, options)
    try:
        tm = judged_exact(t2, R, case)
        print(f"{case}: num_bins {list(tm.num_bins)} nft {t2.stat('nft')}")
        census(t2, tm, A.M)
        if case in se.COPY_CASES:
            kernels = se.numeric_kernels(tm, t2.stat("nft") == 1)
            assert kernels == {f"k_copy_hash<{case.split('_')[2]}>"}, kernels
    finally:
        t2.close()
        A.d_release_csr()
        B.d_release_csr()


# ------------------------------------------------------------------ a speculated second call ---
@pytest.mark.parametrize("name", ["bin_zoo", "run_zoo", "fem_5_5_13"])
def test_repeats_speculated_second_call(tool, name):
    """The same call twice on the same device arrays: the second one queues the first's numeric plan behind the
    scan (a hit), and both results are judged.  (A first call on the merged twin with the twin then copied into
    the same device arrays is not possible: a twin stores more entries than its merge, so nnz never matches.)"""
    R = reference(name)
    A, B, counts = R[0], R[1], R[5]
    assert present(counts) >= kinds_for(name) and len(B.col) > counts["repeated_entries"] > 0
    on_device(tool, A, B)
    t2 = fresh_tool(tool, {}, {})
    try:
        tm1 = judged_exact(t2, R, f"{name}, first call")
        assert t2.stat("spec") == 0
        tm2 = judged_exact(t2, R, f"{name}, speculated second call")
        assert t2.stat("spec") == 1 and t2.stat("spec_miss") == 0, (t2.stat("spec"), t2.stat("spec_miss"))
        assert list(tm1.num_bins) == list(tm2.num_bins)
    finally:
        t2.close()
        A.d_release_csr()
        B.d_release_csr()


# ------------------------------------------------------------------ the mask-formation kernels ---
MASK_LANE_LONG, MASK_LONG, MHS_LANE_AVG = 32, 16, 9  # mhs_kernels.hip, mhs_frontplan.hpp


def mask_kernel(nnzB, MB):
    """mhs_frontplan.hpp's mask_launch: (kernel, variant) for a B of MB rows and nnzB entries."""
    avg = nnzB // MB
    if avg < MHS_LANE_AVG:
        return "k_mask_lane", 4 if avg < 4 else 8
    G = 8
    while 2 * G <= avg // 8 and G < 64:
        G <<= 1
    return "k_mask_b", G


@functools.lru_cache(maxsize=None)
def mask_case(which):
    """A B for one mask-formation kernel, runs of 1..3 adjacent rows with one pattern (kinds g and h need them), its
    twin, and an A that walks consecutive B rows (run walks) and scattered ones.
    lane: rows of 1..9 columns over 3000; the twin adds the rows of 65 and 200 copies of one column and those
    repeated up to the positions 31 / 32 and 63 / 64 -- rows past MASK_LANE_LONG = 32 entries, which the whole wave
    walks.  group: rows of 20..120 columns and a few of 150..300; the twin's longest rows pass MASK_LONG * 8 = 128
    entries and are deferred to the whole wave, the row of 65 copies of one column stays with its 8 lanes."""
    rng = np.random.default_rng(91 if which == "lane" else 92)
    K, N = (1500, 3000) if which == "lane" else (400, 20_000)
    rows = []
    while len(rows) < K:
        if which == "lane":
            ln = int(rng.integers(1, 10))
        else:
            ln = int(rng.integers(150, 301)) if rng.random() < 0.03 else int(rng.integers(20, 121))
        if rng.random() < 0.1:
            ln = 1
        pat = np.sort(rng.choice(N, ln, replace=False))
        rows.extend([pat] * int(rng.integers(1, 4)))
    rows = rows[:K]
    ptr = np.zeros(K + 1, np.int64)
    ptr[1:] = np.cumsum([len(r) for r in rows])
    base = (K, N, ptr.astype(np.int32), np.concatenate(rows).astype(np.int32), np.zeros(int(ptr[-1])))
    twin, counts = with_repeats(base, 5, share=0.05, per_kind=3)
    arows = []
    for i in range(600):
        s = int(rng.integers(0, K - 12))
        arows.append(np.arange(s, s + int(rng.integers(1, 12))) if i % 2 else np.sort(rng.choice(K, int(rng.integers(1, 7)), replace=False)))
    lens = np.diff(twin[2])
    arows += [np.array([k]) for k in np.nonzero(lens > (MASK_LANE_LONG if which == "lane" else 64))[0]]  # every long row is reached
    Ap = np.zeros(len(arows) + 1, np.int64)
    Ap[1:] = np.cumsum([len(r) for r in arows])
    Ac = np.concatenate(arows).astype(np.int32)
    At = (len(arows), K, Ap.astype(np.int32), Ac, edge_values(len(Ac), 8))
    return (*exact_reference(At, twin), counts)


@pytest.mark.parametrize("which", ["lane", "group"])
def test_repeats_mask_formation(tool, which):
    """lane: B averages fewer than MHS_LANE_AVG = 9 entries a row (nnzB / MB < 9, mask_launch), so k_mask_lane forms
    the masks, a lane per row, and rows past MASK_LANE_LONG = 32 entries go to the whole wave's walk.  group: nnzB / MB
    is at least 9 and below 128, so k_mask_b runs with G = 8 lanes a row, and rows past MASK_LONG * G = 128 entries are
    deferred to the whole wave.  Kinds c, d, e and h are in both."""
    R = mask_case(which)
    A, B, counts = R[0], R[1], R[5]
    assert present(counts) >= set("cdeh"), counts
    lens = np.diff(B.ptr)
    kernel = mask_kernel(B.nnz, B.M)
    if which == "lane":
        assert kernel == ("k_mask_lane", 8) and np.count_nonzero(lens > MASK_LANE_LONG) >= 4, (kernel, lens.max())
    else:
        assert kernel == ("k_mask_b", 8), kernel
        assert np.count_nonzero(lens > MASK_LONG * 8) >= 4 and np.count_nonzero((lens > 64) & (lens <= MASK_LONG * 8)) >= 1
    assert counts["longest_tile_run"] >= 200
    reached = np.bincount(A.col, minlength=B.M) > 0
    assert reached[lens > MASK_LANE_LONG].all() if which == "lane" else reached[lens > MASK_LONG * 8].all()
    on_device(tool, A, B)
    t2 = fresh_tool(tool, {}, {})
    try:
        tm = judged_exact(t2, R, f"mask formation, {which}")
        print(f"mask {which}: {kernel}, num_bins {list(tm.num_bins)}")
        assert sum(tm.num_bins[1:]) > 0 and tm.nnzC > 0, tm.num_bins
        judged_exact(t2, R, f"mask formation, {which}, the call repeated")
    finally:
        t2.close()
        A.d_release_csr()
        B.d_release_csr()
