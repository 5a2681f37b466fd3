"""CPU check of tests/_util.py's compress_columns, the reference of the GPU tests whose column space the oracle's
dense arrays cannot take (tests/test_gpu_scale_edges.py): compress B's columns, multiply, expand -- against the
oracle's direct product, at an N it can take."""
import numpy as np

from oracle import oracle as orc
from _util import compress_columns, exact_forward, csr_of, random_csr, tiny_zoo


def test_map_is_monotone_and_invertible():
    col = np.array([7, 7, 2_000_000_000, 64, 63, 2**31 - 2, 64, 0], np.int32)
    ranks, true = compress_columns(col)
    assert ranks.dtype == np.int32 and ranks.shape == col.shape
    assert np.array_equal(true, [0, 7, 63, 64, 2_000_000_000, 2**31 - 2])
    assert np.array_equal(true[ranks], col)
    assert np.array_equal(ranks, [1, 1, 4, 3, 2, 5, 3, 0])
    order = np.argsort(col, kind="stable")
    assert np.all(np.diff(ranks[order]) >= 0), "monotone: sorted columns stay sorted, equal ones equal"
    e, t = compress_columns(np.zeros(0, np.int32))
    assert len(e) == 0 and len(t) == 0


def compressed_product(A, B):
    _, _, Ap, Ac, Av = A
    K, N, Bp, Bc, Bv = B
    ranks, true = compress_columns(Bc)
    assert len(true) < N, "the case compresses"
    Cp, Ci, Cv = orc.spgemm(Ap, Ac, Av, Bp, ranks, Bv, len(true))
    return Cp, true[Ci].astype(np.int32), Cv, (ranks, true)


def cases():
    p, c, v = random_csr(400, 300, 6, seed=3, signed=True)
    Bp, Bc, Bv = random_csr(300, 1_000_000, 9, seed=4, signed=True)  # scattered: ~2700 of 10^6 columns used
    yield (400, 300, p, c, v), (300, 1_000_000, Bp, Bc, Bv)
    p, c, v = random_csr(50, 40, 5, seed=5, sorted_unique=False)      # duplicate and unsorted A entries
    Bp, Bc, Bv = random_csr(40, 90_000, 4, seed=6)
    yield (50, 40, p, c, v), (40, 90_000, Bp, Bc + 64 * 100, Bv)      # ... and a shifted B
    At, Bt = tiny_zoo(7)                                              # colliding columns, empty B rows
    yield At, Bt


def test_compress_multiply_expand_is_the_direct_product():
    for A, B in cases():
        _, _, Ap, Ac, Av = A
        K, N, Bp, Bc, Bv = B
        Dp, Di, Dv = orc.spgemm(Ap, Ac, Av, Bp, Bc, Bv, N)
        Cp, Ci, Cv, (ranks, true) = compressed_product(A, B)
        assert np.array_equal(Cp, Dp) and np.array_equal(Ci, Di), "the pattern, bit for bit"
        assert np.array_equal(Cv, Dv), "the same products in the same order: the same sums"
        # the long-double reference on the compressed B is the one on B
        Ac_, Bx, Bk = csr_of(A), csr_of(B), csr_of((K, len(true), Bp, ranks, Bv))
        ref, m, S = exact_forward(Ac_, Bx, Dp, Di, Av, Bv)
        refc, mc, Sc = exact_forward(Ac_, Bk, Cp, np.searchsorted(true, Ci).astype(np.int32), Av, Bv)
        assert np.array_equal(ref, refc) and np.array_equal(m, mc) and np.array_equal(S, Sc)
