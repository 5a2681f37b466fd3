"""GPU tests of the semiring values plans, their subgradient and their witness on rows placed exactly on every class
edge (min-plus, max-plus and max-min; FP64 and FP32): the ladder the plus-times paths are held to in
tests/test_gpu_edges.py, test_gpu_values_f32.py, test_gpu_values_batched.py, test_gpu_values_mixed.py and
test_gpu_smooth.py, for the paths with the strongest contract of include/mhspgemm.h -- the forward bit-identical to a
sequential evaluation, ties and wit exact integers, and dA and dB exact too on integer values with G = ties * g.

A case (tests/_semiring_edges.py) is EDGE_COPIES rows of _util.edge_val(n, span, products) on one side of one edge of
csrc/mhs_valplan.hpp's val_class: the last slot of a searched slice (padded to an even entry count), the last column
of a direct span (filled with the identity of add in the forward, with NaN in the backward walk), the first row that
leaves a class, the first rows of the global class (min / max atomics into C's segment; its Cval and C.col read in
memory by the three passes of the backward walk).  Everything runs on one plan per case: info(), the forward, both
regimes of tests/test_gpu_subgrad.py and of tests/test_gpu_witness.py as they are, and the one-sided subgradient calls,
whose kernels hold no group sum (wants().wa is false at compile time).  Every comparison is np.array_equal, or the
subgradient's own bound 1.01 (m + 1) u S in its general regime; nothing here introduces a tolerance.  Every output
buffer starts as NaN, ties as -1 and wit as 12345."""
import numpy as np
import pytest

import mhspgemm
import _semiring_edges as se
import test_gpu_semiring as fwd
import test_gpu_subgrad as sub
import test_gpu_witness as wit

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("sr", se.SEMIRINGS)
@pytest.mark.parametrize("dtype", se.DTYPES)
@pytest.mark.parametrize("side", [0, 1], ids=se.SIDES)
@pytest.mark.parametrize("name", se.RUNGS)
def test_semiring_class_edges(tool, name, side, dtype, sr):
    n, span, products, cls = se.rung(name, side, dtype)
    A, B, Cp, Ci, pqs = se.pattern(n, span, products)
    nC = len(Ci)
    # the reference alone, before anything is compared with the device: the case is not empty
    av, bv, c, win, T = exact = se.exact_case(sr, n, span, products, dtype)
    se.conditions(name, sr, n, span, products, dtype, exact)
    what = f"{name} {se.SIDES[side]} {sr} {dtype}"
    dA, dB, dC = fwd.on_device(tool, A, B, Cp, Ci)
    plan = mhspgemm.ValuesPlan(tool, dA, dB, dC, dtype=dtype, semiring=sr)
    try:
        info = plan.info()
        classes = [k for k in range(8) if info["rows"][k]]
        assert sum(info["rows"]) == A.M and classes == [cls] == [se.val_class(n, span, products, se.SUM_BYTES[dtype])], info
        assert fwd.same_classes(info, fwd.plus_times_info(tool, dA, dB, dC, dtype)), "semirings do not move classes"
        # the forward, into a NaN-filled output
        cdev = sub.forward_values(tool, plan, nC, dtype, av, bv)
        got = cdev.cpu().numpy()
        assert got.dtype == fwd.NP[dtype] and np.array_equal(got, c), f"{what}: the forward"
        # the subgradient and the witness, both regimes
        assert np.array_equal(sub.check_exact(tool, plan, A, B, nC, pqs, sr, dtype, se.SEED), T)
        sub.check_general(tool, plan, A, B, nC, pqs, sr, dtype, se.SEED + 7, what)
        wit.check_exact(tool, plan, A, B, nC, pqs, sr, dtype, se.SEED)
        wit.check_general(tool, plan, A, B, nC, pqs, sr, dtype, se.SEED + 7)
        # every entry of wit is written, and an entry has a witness exactly where it has winners
        g = np.random.default_rng(se.SEED + 1).integers(-2, 3, nC).astype(np.float64)
        G = np.where(T > 0, T * g, np.nan)
        _, gA, gB, ties = sub.call(tool, plan, A.nnz, B.nnz, nC, dtype, av, bv, G, cval=cdev)
        _, w = wit.call(tool, plan, nC, dtype, av, bv, cval=cdev)
        assert not (w == wit.JUNK).any() and np.all(w >= -1) and np.all(w < A.N), f"{what}: every entry of wit is written"
        assert np.array_equal(ties, T) and np.array_equal(w >= 0, ties >= 1), f"{what}: a witness exactly where ties >= 1"
        # one-sided calls: other kernels (no group sum without dA), the same results
        wA, wB = sub.exact_reference(sr, pqs, win, T, av, bv, G, A.nnz, B.nnz, dtype)
        assert np.array_equal(gA, wA) and np.array_equal(gB, wB)
        _, oA, xB, tA = sub.call(tool, plan, A.nnz, B.nnz, nC, dtype, av, bv, G, cval=cdev, need_B=False)
        _, xA, oB, tB = sub.call(tool, plan, A.nnz, B.nnz, nC, dtype, av, bv, G, cval=cdev, need_A=False)
        assert np.isnan(xA).all() and np.isnan(xB).all(), f"{what}: the side not asked for keeps its bytes"
        assert oA.tobytes() == gA.tobytes(), f"{what}: dA alone has the bytes of the two-sided call's"
        assert np.array_equal(oB, gB) and np.array_equal(oB, wB), f"{what}: dB alone has the values of the two-sided call's"
        assert np.array_equal(tA, T) and np.array_equal(tB, T), f"{what}: ties of the one-sided calls"
    finally:
        plan.close()
