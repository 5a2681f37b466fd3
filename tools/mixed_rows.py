"""mixed_rows.py -- for the bench tools' checks of a mixed values plan (float32 values, float64 sums): which rows of a C
pattern such a plan sends to its global class, whose sums stay float and whose entries therefore have the float32 bound.
The rule is csrc/mhs_valplan.hpp's at 8 * width sum bytes, restated; every tool that uses it holds its count against
the plan's own ``info()["global"]``."""
import numpy as np

VAL_BLOCK_BYTES = 159744  # (mhs_valplan.hpp: the dynamic LDS of the block classes)


def mixed_global_rows(ptr, col, width=1):
    """Per row of the host pattern (ptr, col): more entries than a block's searched slice holds, over more columns than
    its direct slice does.  Rows without products (all zeros) and a masked plan's dot rows (double sums) aside."""
    ptr, col = np.asarray(ptr, np.int64), np.asarray(col, np.int64)
    assert width in (1, 2, 4)
    sb = 8 * width
    n = np.diff(ptr)
    has = n > 0
    span = np.zeros(len(n), np.int64)
    span[has] = col[ptr[1:][has] - 1] - col[ptr[:-1][has]] + 1
    return (n > (VAL_BLOCK_BYTES // (sb + 4) & ~1)) & (span > VAL_BLOCK_BYTES // sb)
