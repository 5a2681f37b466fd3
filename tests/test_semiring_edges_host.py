"""Host tests of the semiring class-edge ladder's inputs (tests/_semiring_edges.py): the conditions that
tests/test_gpu_semiring_edges.py asserts before it compares anything with the device, over all of its cases, so that
they are held without a GPU -- a case must not pass by being empty.  Everything here is the numpy reference of
tests/test_gpu_subgrad.py (exact_values, winners) and tests/test_gpu_semiring.py (reference)."""
import numpy as np
import pytest

import _semiring_edges as se
from _util import EDGE_COPIES


@pytest.mark.parametrize("sr", se.SEMIRINGS)
@pytest.mark.parametrize("dtype", se.DTYPES)
@pytest.mark.parametrize("side", [0, 1], ids=se.SIDES)
@pytest.mark.parametrize("name", se.RUNGS)
def test_edge_case_conditions(name, side, dtype, sr):
    n, span, products, cls = se.rung(name, side, dtype)
    assert cls == se.val_class(n, span, products, se.SUM_BYTES[dtype]), "the table's class is the Python mirror's"
    counts = se.conditions(name, sr, n, span, products, dtype, se.exact_case(sr, n, span, products, dtype))
    print(f"{name} {se.SIDES[side]} {dtype} {sr}: (n, span, products) = {(n, span, products)}, entries with ties {counts[0]}, "
          f"last entries won {counts[1]} of {EDGE_COPIES}, reached entries without a winner {counts[2]}")


def test_edge_cases_straddle_every_edge():
    """The two sides of a rung differ by one in one parameter and lie in different classes; the largest row has
    19,969 entries: nothing here needs a workload-sized matrix."""
    largest = 0
    for dtype in se.DTYPES:
        for name in se.RUNGS:
            at, above = se.rung(name, 0, dtype), se.rung(name, 1, dtype)
            assert at[3] != above[3], (name, dtype)
            assert sorted(abs(x - y) for x, y in zip(at[:3], above[:3])) == [0, 0, 1], (name, dtype)
            largest = max(largest, at[0], above[0])
    assert largest == 19969


def test_float32_exact_regime_is_the_float64_one():
    """Integers in [-3, 3] and infinities: rounding the values to float32 changes no product, so one set of conditions
    covers both types (the team rungs are one input for both)."""
    n, span, products, _ = se.rung("wave_search_n", 0, "float32")
    for sr in se.SEMIRINGS:
        c64, c32 = (se.exact_case(sr, n, span, products, dtype) for dtype in se.DTYPES)
        assert c32[2].dtype == np.float32 and np.array_equal(c64[2], c32[2]) and np.array_equal(c64[4], c32[4])
