"""Host tests of the repeat twins (tests/_dups.py): the inputs of tests/test_gpu_b_repeats*.py, and the reference's
own reading of "duplicates in A or B are summed" (include/mhspgemm.h), held without a GPU.

For the twins of bin_zoo, tiny_zoo(7), run_zoo(5), group_zoo(3) and near_zoo, and for the aliased A * A cases: the
twin is legal input (rows ascending, columns in range), holds every kind of repeat its input can take -- all of a..i
where the input has two pairs of adjacent rows with one pattern; bin_zoo and tiny_zoo have none, so no twin of theirs
can hold g or h, and the uniform FEM cases leave e, f and h out by design (_dups.ALIASED) -- and merges back into
the input's pattern; the oracle's C on (A, twin) is its C on (A, merged twin) bit for bit; expand() on the twin
yields orc.flop products, each with a slot.  Values are integers of +-{1, 2, 3}: every comparison is an equality."""
import functools

import numpy as np
import pytest

from oracle import oracle as orc
from _dups import (ALIASED, KINDS, NUM_WS_WORK, RUNS, UNIFORM, ZOO_NAMES, can_hold, integer_values, is_legal,
                   magnitudes_differ, max_products, merge_repeats, present, repeat_kinds, row_products, twin_operands,
                   with_repeats)
from _util import edge_values, expand

CASES = list(ZOO_NAMES) + list(ALIASED)


def test_with_repeats_by_hand():
    """Rows of 1, 1, 1, 3, 3, 3, 3, 3, 6 and 70 entries: every kind lands, the twin merges back, a second call with
    the seed gives the same twin, and repeat_kinds reads the kinds of a hand-written matrix."""
    rows = [[5], [9], [70], [1, 2, 3], [1, 2, 3], [1, 2, 3], [1, 2, 3], [1, 2, 3], [10, 63, 64, 65, 200, 300], list(range(100, 170))]
    rows += [[7, 8, 9, 10, 11, 12]] * 4 + [[20, 21, 22, 23, 24, 25, 26]] * 6 + [list(range(400, 440))] * 3
    rows += [list(range(k, k + 9)) for k in range(0, 200, 10)]
    ptr = np.zeros(len(rows) + 1, np.int32)
    ptr[1:] = np.cumsum([len(r) for r in rows])
    col = np.concatenate(rows).astype(np.int32)
    Bt = (len(rows), 500, ptr, col, edge_values(len(col), 1))
    assert can_hold(Bt) == set(KINDS)
    twin, counts = with_repeats(Bt, 3, share=0.3)
    again, _ = with_repeats(Bt, 3, share=0.3)
    assert all(np.array_equal(x, y) for x, y in zip(twin[2:], again[2:]))
    assert is_legal(twin) and integer_values(twin[4]) and magnitudes_differ(twin)
    assert present(counts) == set(KINDS), counts
    assert all(counts[f"e_single_{r}"] == 1 for r in RUNS), counts
    m = merge_repeats(twin)
    assert np.array_equal(m[2], ptr) and np.array_equal(m[3], col)
    hand = (3, 200, np.array([0, 3, 6, 11], np.int32), np.array([1, 1, 2, 1, 2, 2, 63, 63, 64, 64, 64], np.int32), np.ones(11))
    c = repeat_kinds(hand)
    assert (c["h"], c["g"], c["d"], c["d_exact"], c["b_first"], c["b_last"]) == (1, 0, 1, 1, 2, 2), c
    mh = merge_repeats(hand)
    assert np.array_equal(mh[2], [0, 2, 4, 6]) and np.array_equal(mh[3], [1, 2, 1, 2, 63, 64]) and np.array_equal(mh[4], [2, 1, 1, 2, 2, 3])
    assert not is_legal((1, 10, np.array([0, 2], np.int32), np.array([3, 2], np.int32), np.ones(2)))
    assert not is_legal((1, 3, np.array([0, 2], np.int32), np.array([2, 3], np.int32), np.ones(2)))


@functools.lru_cache(maxsize=None)
def products(name):
    """The case's operands as (At, Bt) tuples, the oracle's C on them and on the merged twin."""
    At, Bt, counts, base = twin_operands(name)
    Bt = At if Bt is None else Bt
    Bm = merge_repeats(Bt)
    Am = Bm if name in ALIASED else At
    C = orc.spgemm(At[2], At[3], At[4], Bt[2], Bt[3], Bt[4], Bt[1])
    Cm = orc.spgemm(Am[2], Am[3], Am[4], Bm[2], Bm[3], Bm[4], Bm[1])
    return At, Bt, C, Cm


@pytest.mark.parametrize("name", CASES)
def test_twin_is_legal_and_holds_every_kind(name):
    At, Bt, counts, base = twin_operands(name)
    twin = At if Bt is None else Bt
    assert is_legal(twin) and integer_values(twin[4]) and integer_values(At[4]) and magnitudes_differ(twin)
    assert len(twin[3]) > len(base[3])
    m = merge_repeats(twin)
    assert np.array_equal(m[2], base[2]) and np.array_equal(m[3], base[3]), "merging gives back the input's pattern"
    assert counts == {**repeat_kinds(twin), "i": counts["i"]}
    have = present(counts)
    print(name, counts)
    if name in UNIFORM:  # (e, f, h left out: _dups.ALIASED says why; g comes with the node triples)
        assert have == set("abcdgi"), (have, counts)
        assert counts["d_exact"] >= 1 and row_products(twin, twin).max() <= NUM_WS_WORK, "the rows stay in the small wave bins"
    else:
        assert have == can_hold(base), (have, counts)
        assert have >= set("abcdefi")
        if name in ("run_zoo", "group_zoo", "near_zoo", "perturbed_fem", "fem_5_5_13_ragged"):
            assert have == set(KINDS)
        if name in ("tiny_zoo", "run_zoo", "group_zoo"):  # matrices with rows of one entry: one column r times is a whole row
            assert all(counts[f"e_single_{r}"] >= 1 for r in RUNS), counts
    assert counts["longest_tile_run"] > 64 or name in UNIFORM


def test_every_kind_occurs_over_the_zoos():
    have = set()
    for name in ZOO_NAMES:
        have |= present(twin_operands(name)[2])
    assert have == set(KINDS)


@pytest.mark.parametrize("name", CASES)
def test_oracle_sums_repeats(name):
    """orc.spgemm on the twin against orc.spgemm on the merged twin: ptr, col and the values, bit for bit."""
    At, Bt, (Cp, Ci, Cv), (Mp, Mi, Mv) = products(name)
    assert np.array_equal(Cp, Mp) and np.array_equal(Ci, Mi)
    # (equal as numbers: a merged entry whose repeats cancel, 1 + 2 - 3, is a stored 0.0, and a negative A value
    # times it is -0.0 where the twin's own sum is +0.0 -- the one difference in bits, and not one in value)
    assert np.array_equal(Cv, Mv) and np.all(Cv == np.round(Cv))
    nz = Mv != 0.0
    assert np.array_equal(Cv[nz].view(np.uint64), Mv[nz].view(np.uint64))
    assert orc.flop(At[3], Bt[2]) > orc.flop(At[3], merge_repeats(Bt)[2])


@pytest.mark.parametrize("name", ZOO_NAMES)
def test_a_mispaired_repeat_changes_the_product(name):
    """What the different magnitudes are for: a product that takes the first copy of every repeated entry twice and
    the second never is another product -- in every row of C that a repeated B entry reaches, bar cancellations."""
    At, Bt, (Cp, Ci, Cv), _ = products(name)
    K, N, ptr, col, val = Bt
    rows = np.repeat(np.arange(K), np.diff(ptr))
    second = np.nonzero((col[1:] == col[:-1]) & (rows[1:] == rows[:-1]))[0] + 1
    wrong = val.copy()
    wrong[second] = wrong[second - 1]
    Wp, Wi, Wv = orc.spgemm(At[2], At[3], At[4], ptr, col, wrong, N)
    assert np.array_equal(Wp, Cp) and np.array_equal(Wi, Ci)
    crow = np.repeat(np.arange(At[0]), np.diff(Cp))
    touched = np.bincount(np.repeat(np.arange(At[0]), np.diff(At[2])), np.isin(At[3], rows[second]), At[0]) > 0
    differs = np.bincount(crow, Wv != Cv, At[0]) > 0
    assert not differs[~touched].any() and touched.sum() > 0
    assert differs[touched].sum() >= 0.9 * touched.sum(), (differs[touched].sum(), touched.sum())


@pytest.mark.parametrize("name", CASES)
def test_expand_reaches_every_product(name):
    At, Bt, (Cp, Ci, Cv), _ = products(name)
    p, q, s = expand(At[2], At[3], Bt[2], Bt[3], Cp, Ci, Bt[1])
    assert len(p) == orc.flop(At[3], Bt[2]) == row_products(At, Bt).sum(), "every product has a slot"
    assert np.array_equal(np.bincount(s, At[4][p] * Bt[4][q], len(Ci)), Cv)
    assert np.bincount(s, minlength=len(Ci)).min(initial=1) >= 1
    assert 9 * max_products(s, len(Ci)) < 2 ** 24, "exact in float as well"


def test_scipy_agrees_on_a_small_twin():
    sp = pytest.importorskip("scipy.sparse")
    At, Bt, (Cp, Ci, Cv), _ = products("tiny_zoo")
    A = sp.csr_matrix((At[4], At[3], At[2]), shape=(At[0], At[1]))
    B = sp.csr_matrix((Bt[4], Bt[3], Bt[2]), shape=(Bt[0], Bt[1]))
    S = (A @ B).tocsr()
    S.sum_duplicates()
    S.sort_indices()
    dense_rows = np.repeat(np.arange(At[0]), np.diff(Cp))
    assert np.array_equal(np.asarray(S[dense_rows, Ci]).ravel(), Cv)
    assert S.nnz <= len(Ci)  # (scipy may drop entries that cancel; the oracle keeps structural zeros)
