"""Shared test helpers (test infrastructure)."""
from __future__ import annotations

import functools
import json
from pathlib import Path

import numpy as np

GOLDEN = Path(__file__).resolve().parent / "golden"


def load_golden(name: str):
    d = json.loads((GOLDEN / f"{name}.json").read_text())
    ptr = np.asarray(d["ptr"], np.int32)
    col = np.asarray(d["col"], np.int32)
    val = np.asarray([float.fromhex(x) for x in d["val_hex"]], np.float64)
    return d, ptr, col, val


PRODUCT_CASES = ["cage4_like", "tile_edges", "dense_row_col", "duplicates", "rect_AB", "empty_product"]
READ_CASES = ["mm_symmetric", "mm_skew", "mm_hermitian", "mm_pattern", "mm_integer", "mm_dups_comments"]


def csr_from_arrays(M, N, ptr, col, val):
    import mhspgemm
    return mhspgemm.CSR(M, N, ptr, col, val)


def random_csr(M, N, per_row, seed, lo=0.1, hi=1.0, sorted_unique=True, signed=False):
    rng = np.random.default_rng(seed)
    lens = rng.poisson(per_row, M)
    rows = np.repeat(np.arange(M), lens)
    cols = rng.integers(0, N, len(rows))
    key = np.unique(rows.astype(np.int64) * N + cols) if sorted_unique else rows.astype(np.int64) * N + cols
    r = key // N
    c = (key % N).astype(np.int32)
    ptr = np.zeros(M + 1, np.int64)
    np.cumsum(np.bincount(r, minlength=M), out=ptr[1:])
    v = rng.uniform(lo, hi, len(c))
    if signed:
        v *= rng.choice([-1.0, 1.0], len(c))
    return ptr.astype(np.int32), c, v


def bin_zoo(seed: int = 11):
    """A (rows of every kind) x B (K x N, N = 2M columns) such that rows land in
    every symbolic and numeric bin, including both global-memory fallbacks:
    empty, single product, banded (direct tables), scattered (hashed tables)
    of growing size, heavy work on a tiny pattern (duplicate A entries)."""
    rng = np.random.default_rng(seed)
    N = 2_000_000
    K = 3000
    # B rows: 0..499 tile [0, 32000) with 64 consecutive cols each, 500..999 "band" (64 consecutive
    # cols, 1000 apart), 1000..2998 "scatter" (50 random cols), row 2999 single entry
    Brows, Bcols = [], []
    for k in range(K):
        if k == K - 1:
            cs = np.array([12345])
        elif k < 500:                                # contiguous tiling of [0, 32000)
            cs = np.arange(64 * k, 64 * k + 64)
        elif k < 1000:
            off = 1000 * k % (N - 64)
            cs = np.arange(off, off + 64)
        else:
            cs = np.unique(rng.integers(0, N, 50))
        Brows.append(np.full(len(cs), k))
        Bcols.append(cs)
    Br = np.concatenate(Brows)
    Bc = np.concatenate(Bcols)
    Bkey = Br.astype(np.int64) * N + Bc
    order = np.argsort(Bkey, kind="stable")
    Br, Bc = Br[order], Bc[order]
    Bptr = np.zeros(K + 1, np.int64)
    np.cumsum(np.bincount(Br, minlength=K), out=Bptr[1:])
    Bv = rng.uniform(0.1, 1.0, len(Bc))

    arows = []  # list of lists of k (A entries, in order, duplicates allowed)
    arows.append([])                                 # empty
    arows.append([K - 1])                            # single product
    for i in range(20):                              # banded, small: direct, wave
        s = int(rng.integers(0, 990))
        arows.append(list(range(s, s + 8)))
    for i in range(10):                              # scattered small: hash, wave
        arows.append(sorted(rng.choice(np.arange(1000, K - 1), 2, replace=False).tolist()))
    for i in range(10):                              # scattered small-medium: hash, 16 KiB wave
        arows.append(sorted(rng.choice(np.arange(1000, K - 1), 4, replace=False).tolist()))
    for nb in (1, 3, 6, 9):                          # scattered rows of 50..450 products (tiny classes)
        for i in range(4):
            arows.append(sorted(rng.choice(np.arange(1000, K - 1), nb, replace=False).tolist()))
    for i in range(4):                               # > 512 products, 50 tiles: hash, wave
        arows.append([int(rng.integers(1000, K - 1))] * 12)
    for i in range(4):                               # > 512 products, ~300 tiles: hash, 256-thread block
        arows.append(sorted(rng.choice(np.arange(1000, K - 1), 6, replace=False).tolist() * 2))
    for i in range(4):                               # > 512 products, ~200 tiles: hash, 10 KiB wave
        arows.append(sorted(rng.choice(np.arange(1000, K - 1), 4, replace=False).tolist() * 3))
    for i in range(6):                               # scattered medium: hash, 256-thread block
        arows.append(sorted(rng.choice(np.arange(1000, K - 1), 20, replace=False).tolist()))
    for i in range(4):                               # scattered large: 1024-thread block
        arows.append(sorted(rng.choice(np.arange(1000, K - 1), 60, replace=False).tolist()))
    for i in range(2):                               # scattered huge: global memory
        arows.append(sorted(rng.choice(np.arange(1000, K - 1), 400, replace=False).tolist()))
    arows.append([5] * 3000)                         # heavy work, tiny pattern (duplicates)
    arows.append(list(range(0, 330)))                # 21120 contiguous columns, direct: global memory
    arows.append(sorted(rng.choice(np.arange(1000, K - 1), 120, replace=False).tolist()))  # wide: 1024 block
    arows.append(sorted(rng.choice(np.arange(0, 1000), 200, replace=False).tolist()))  # wide banded
    arows.append(list(range(0, 1000, 3)))            # direct, large span
    M = len(arows)
    Aptr = np.zeros(M + 1, np.int64)
    Aptr[1:] = np.cumsum([len(r) for r in arows])
    Acol = np.array([k for r in arows for k in r], np.int32)
    Av = rng.uniform(0.1, 1.0, len(Acol))
    return (M, K, Aptr.astype(np.int32), Acol, Av), (K, N, Bptr.astype(np.int32), Bc.astype(np.int32), Bv)


def run_zoo(seed: int = 5, N: int = 40_000):
    """B whose rows come in groups sharing one column pattern (runs of 1..7 rows,
    like the dofs of a FEM node), plus decoys: adjacent rows of equal length but
    different columns, and empty rows.  A rows walk consecutive B rows (runs, cut
    at 64-entry chunk edges and at the 3-row merge cap), skip rows (runs broken),
    repeat a row (k, k: not a run) and are long enough to reach the block and
    global kernels.  Exercises the same-pattern flag of the mask formation and the
    run walks of the symbolic and numeric phases."""
    rng = np.random.default_rng(seed)
    rows = []
    while len(rows) < 4000:
        kind = rng.integers(0, 10)
        if kind == 0:
            rows.append(np.zeros(0, np.int64))                       # empty row
            continue
        ln = int(rng.integers(1, 120))
        pat = np.unique(rng.integers(0, N, ln))
        if kind == 1:                                                # decoy: same length, new cols
            rows.append(pat)
            alt = np.unique(rng.integers(0, N, 4 * len(pat)))[:len(pat)]
            rows.append(np.sort(alt))
            continue
        rows.extend([pat] * int(rng.integers(1, 8)))                 # a run of 1..7 equal rows
    K = len(rows)
    Bptr = np.zeros(K + 1, np.int64)
    Bptr[1:] = np.cumsum([len(r) for r in rows])
    Bc = np.concatenate(rows).astype(np.int32)
    Bv = rng.uniform(0.1, 1.0, len(Bc))
    arows = []
    for i in range(600):
        kind = i % 6
        s = int(rng.integers(0, K - 400))
        if kind == 0:
            arows.append(list(range(s, s + int(rng.integers(1, 40)))))          # wave bins
        elif kind == 1:
            arows.append(list(range(s, s + int(rng.integers(60, 140)))))        # crosses chunk edges
        elif kind == 2:
            arows.append(sorted(set(rng.integers(s, s + 60, 30).tolist())))     # runs broken by gaps
        elif kind == 3:
            arows.append([s, s, s + 1, s + 1, s + 2])                           # repeats: not runs
        elif kind == 4:
            arows.append(list(range(s, s + 390)))                               # block / global kernels
        else:
            arows.append([])
    M = len(arows)
    Aptr = np.zeros(M + 1, np.int64)
    Aptr[1:] = np.cumsum([len(r) for r in arows])
    Acol = np.array([k for r in arows for k in r], np.int32)
    Av = rng.uniform(0.1, 1.0, len(Acol))
    return (M, K, Aptr.astype(np.int32), Acol, Av), (K, N, Bptr.astype(np.int32), Bc, Bv)


def group_zoo(seed: int = 3, K: int = 6000, N: int = 30_000):
    """A whose rows repeat column patterns (runs of 1..8 equal rows, so row groups of
    1..3 and runs cut by the group size and by the 96-row breaks), with small,
    medium and large patterns (grouped wave bins, the 16 KiB grouped bin, and
    groups too large for any grouped bin that run row by row); B random (K x N)
    with some same-pattern row runs of its own.  Values differ per row."""
    rng = np.random.default_rng(seed)
    arows = []
    while len(arows) < 700:
        size = int(rng.choice([2, 6, 20, 60, 200]))
        pat = np.unique(rng.integers(0, K, size))
        arows.extend([pat] * int(rng.integers(1, 9)))
        if rng.random() < 0.1:
            arows.append(np.zeros(0, np.int64))  # an empty row breaks a run
    M = len(arows)
    Aptr = np.zeros(M + 1, np.int64)
    Aptr[1:] = np.cumsum([len(r) for r in arows])
    Acol = np.concatenate(arows).astype(np.int32)
    Av = rng.uniform(0.1, 1.0, len(Acol))
    brows = []
    while len(brows) < K:
        pat = np.unique(rng.integers(0, N, int(rng.integers(1, 40))))
        brows.extend([pat] * int(rng.integers(1, 4)))
    brows = brows[:K]
    Bptr = np.zeros(K + 1, np.int64)
    Bptr[1:] = np.cumsum([len(r) for r in brows])
    Bc = np.concatenate(brows).astype(np.int32)
    Bv = rng.uniform(0.1, 1.0, len(Bc))
    return (M, K, Aptr.astype(np.int32), Acol, Av), (K, N, Bptr.astype(np.int32), Bc, Bv)


def tiny_zoo(seed: int = 7, K: int = 3000, N: int = 5000):
    """Rows for every tiny class (team of W lanes x K products per lane: flop <= 8, 32, 64
    with nA <= 8; <= 32, 64, 128 with nA <= 32; <= 256, 512 with nA <= 64), with colliding
    columns (B rows drawn from a narrow column window, repeated A entries) so segments of
    equal columns span lanes and slots, plus rows just past the limits (flop 513+, nA
    past the lane count with empty B rows)."""
    rng = np.random.default_rng(seed)
    brows = []
    for k in range(K):
        kind = k % 5
        if kind == 0:
            brows.append(np.zeros(0, np.int64))                                     # empty B row
        elif kind == 1:
            brows.append(np.unique(rng.integers(0, 200, int(rng.integers(1, 4)))))  # narrow: collisions
        else:
            brows.append(np.unique(rng.integers(0, N, int(rng.integers(1, 9)))))
    Bptr = np.zeros(K + 1, np.int64)
    Bptr[1:] = np.cumsum([len(r) for r in brows])
    Bc = np.concatenate(brows).astype(np.int32)
    Bv = rng.uniform(0.1, 1.0, len(Bc))
    blen = np.diff(Bptr)
    nonempty = np.nonzero(blen)[0]
    empty = np.nonzero(blen == 0)[0]
    arows = []
    for target, amax in ((1, 8), (4, 8), (8, 8), (16, 8), (30, 8), (32, 8), (60, 8), (64, 8), (20, 32), (32, 32),
                         (50, 32), (64, 32), (100, 32), (128, 32),
                         (129, 32), (200, 64), (256, 64), (300, 64), (512, 64), (513, 64), (700, 64)):
        for _ in range(30):
            ks, f = [], 0
            for _try in range(600):
                if f >= target or len(ks) >= amax:
                    break
                k = int(rng.choice(nonempty))
                if f + blen[k] > target:
                    continue
                ks.append(k)
                f += int(blen[k])
                if rng.random() < 0.2 and f + blen[k] <= target and len(ks) < amax:
                    ks.append(k)  # repeated A entry: every product collides
                    f += int(blen[k])
            arows.append(sorted(ks))
    for na in (34, 66):  # many A entries, few products: past a class's lane count
        for _ in range(15):
            arows.append(sorted(rng.choice(empty, na, replace=False).tolist() + [int(rng.choice(nonempty))]))
    arows.append([])
    M = len(arows)
    Aptr = np.zeros(M + 1, np.int64)
    Aptr[1:] = np.cumsum([len(r) for r in arows])
    Acol = np.array([k for r in arows for k in r], np.int32)
    Av = rng.uniform(0.1, 1.0, len(Acol))
    return (M, K, Aptr.astype(np.int32), Acol, Av), (K, N, Bptr.astype(np.int32), Bc, Bv)


def near_zoo(seed: int = 4):
    """A x B for near row groups (GRP_NEAR): B a 27-point x 3-dof FEM grid, A its pattern
    with 5 % of the off-diagonal entries dropped per row (dof triples whose A rows differ
    by a few entries but whose C rows mostly coincide), and some rows made awkward: a far
    column appended (unsorted, and the row's C pattern no longer matches its triple's), an
    entry repeated (a duplicate column, summed), the row reversed (unsorted A)."""
    from mhspgemm import synth
    B = synth.fem_grid(12, 10, 8, seed=seed)
    rng = np.random.default_rng(seed)
    cols, vals, lens = [], [], []
    for i in range(B.M):
        c = B.col[B.ptr[i]:B.ptr[i + 1]].copy()
        v = rng.uniform(0.1, 1.0, len(c))
        keep = (c == i) | (rng.random(len(c)) >= 0.05)
        c, v = c[keep], v[keep]
        u = rng.random()
        if u < 0.04:
            c = np.append(c, rng.integers(0, B.M))
            v = np.append(v, 0.5)
        elif u < 0.07:
            j = int(rng.integers(0, len(c)))
            c = np.insert(c, j, c[j])
            v = np.insert(v, j, 0.25)
        elif u < 0.10:
            c, v = c[::-1].copy(), v[::-1].copy()
        cols.append(c)
        vals.append(v)
        lens.append(len(c))
    ptr = np.zeros(B.M + 1, np.int64)
    ptr[1:] = np.cumsum(lens)
    A = (B.M, B.M, ptr.astype(np.int32), np.concatenate(cols).astype(np.int32), np.concatenate(vals))
    return A, (B.M, B.N, B.ptr, B.col, B.val)


def with_hub_row(ptr, col, N, n_hub, feed=0):
    """A pattern changed in place: the same M and nnz, so it fits the device arrays of (ptr, col).  Row 0 becomes a
    hub row of n_hub columns (its own and every other column of [0, N) until there are n_hub), paid for by
    shortening the last rows; rows 1..feed get 0 as their first column, so in A*A their C rows take the hub's."""
    M = len(ptr) - 1
    rows = [col[ptr[i]:ptr[i + 1]] for i in range(M)]
    hub = np.unique(np.concatenate([rows[0], np.arange(0, N, 2)]))[:n_hub]
    extra = len(hub) - len(rows[0])
    rows[0] = hub
    i = M - 1
    while extra > 0:
        take = min(extra, len(rows[i]))
        rows[i] = rows[i][:len(rows[i]) - take]
        extra -= take
        i -= 1
    assert i > feed, "the shortened rows stay clear of the fed ones"
    for r in range(1, feed + 1):
        if len(rows[r]):
            rows[r] = rows[r].copy()
            rows[r][0] = 0
    p2 = np.zeros(M + 1, np.int64)
    np.cumsum([len(r) for r in rows], out=p2[1:])
    c2 = np.concatenate(rows).astype(np.int32)
    assert len(c2) == len(col) and p2[-1] == ptr[-1]
    return p2.astype(np.int32), c2


def compress_columns(col):
    """B's columns mapped to their ranks among the distinct columns used: (ranks, true), ranks an int32 array of
    col's shape, true the sorted distinct columns, true[ranks] == col.  The map is monotone, so sortedness,
    duplicates and the product's structure are kept: the C of A * (B with the ranks, N = len(true)) is the C of
    A * B with every column index c replaced by true[c].  For column spaces the oracle's dense per-thread arrays
    of N entries cannot take (N up to INT32_MAX)."""
    true, ranks = np.unique(np.asarray(col), return_inverse=True)
    return ranks.reshape(np.shape(col)).astype(np.int32), true


# ---------------------- helpers of the values-plan GPU tests (values, masked, backward) ---
RTOL, ATOL = 1e-6, 1e-12  # the project's value tolerance (tests/test_gpu_parity.py)


def new_values(n, seed, signed=False):
    rng = np.random.default_rng(seed)
    v = rng.uniform(0.1, 1.0, n)
    if signed:
        v *= rng.choice([-1.0, 1.0], n)
    return v


def upload(tool, v):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)).to(f"cuda:{tool.device}")
    torch.cuda.synchronize()
    return t


def filled(tool, n, value=float("nan")):
    import torch
    out = torch.full((n,), value, dtype=torch.float64, device=f"cuda:{tool.device}")
    torch.cuda.synchronize()
    return out


def csr_of(t):
    import mhspgemm
    M, N, p, c, v = t
    return mhspgemm.CSR(M, N, p, c, v)


def device_csr(tool, M, N, ptr, col, val=None):
    import mhspgemm
    X = mhspgemm.CSR(M, N, ptr, col, np.zeros(len(col)) if val is None else val)
    X.H2D(tool.device)
    return X


def assert_values(Cp, Ci, Cv, p, c, v, absv=None):
    """(p, c, v) is (Cp, Ci, Cv): the pattern exactly, every value written, and within 1e-6 relative / 1e-12
    absolute and the reference's 1e-9 rule -- or, with mixed signs, 1e-6 of the product on absolute values."""
    import mhspgemm
    from oracle import oracle as orc
    assert np.array_equal(p, Cp) and np.array_equal(c, Ci), "the pattern is C's own"
    assert v.shape == Cv.shape and not np.isnan(v).any(), "every entry is written"
    if absv is not None:
        assert np.all(np.abs(v - Cv) <= 1e-6 * absv + 1e-300)
        return
    ok, _, _, bv, mr = mhspgemm.compare_tol(Cp, Ci, Cv, p, c, v, RTOL, ATOL)
    assert ok, f"{bv} values outside 1e-6 relative (max {mr:.3e})"
    assert orc.compare_ref(Cp, Ci, Cv, p, c, v) == 1, "reference 1e-9 rule"


# ------------------------------------------- the values backward's reference ---
def keys(ptr, col, N):
    rows = np.repeat(np.arange(len(ptr) - 1, dtype=np.int64), np.diff(ptr))
    return rows * N + col


def expand(Ap, Ac, Bp, Bc, Cp, Ci, N):
    """Every product of A*B whose column is in its C row, as index arrays: A entry p, B entry q, C slot s."""
    lens = (Bp[Ac.astype(np.int64) + 1] - Bp[Ac.astype(np.int64)]).astype(np.int64)
    p = np.repeat(np.arange(len(Ac), dtype=np.int64), lens)
    q = np.repeat(Bp[Ac.astype(np.int64)].astype(np.int64), lens) + (np.arange(lens.sum()) - np.repeat(np.cumsum(lens) - lens, lens))
    i = np.repeat(np.arange(len(Ap) - 1, dtype=np.int64), np.diff(Ap))[p]
    kC = keys(Cp, Ci, N)
    if len(kC) == 0 or len(p) == 0:
        e = np.zeros(0, np.int64)
        return e, e, e
    key = i * N + Bc[q]
    s = np.minimum(np.searchsorted(kC, key), len(kC) - 1)
    hit = kC[s] == key
    return p[hit], q[hit], s[hit]


def ref_grad(pqs, av, bv, G, nnzA, nnzB):
    p, q, s = pqs
    return np.bincount(p, bv[q] * G[s], nnzA), np.bincount(q, av[p] * G[s], nnzB)


# ------------------------------------------------- the FP64 rounding bound ---
# The contract of every FP64 value path (include/mhspgemm.h): an output entry summed from m kept products, S the
# sum of their absolute values, is within gamma_m * S of the exact sum, gamma_m = m u / (1 - m u), u = 2^-53 --
# the any-order bound of a float64 sum of m rounded (or fused) products, whether the sum runs in LDS, through
# global atomics, over lanes or sequentially.  The tests hold 1.01 * m * 2^-53 * S: the 1.01 covers gamma_m
# against m u (m < 2^20) and the reference's own error, m * 2^-64 * S in long double (2^-11 of the bound).  It
# is the factor of tests/test_gpu_values_f32.py; no number in it is measured.  The explicit 0 * b products that
# near groups and union rows add are exact and do not count in m.  m = 0: exactly 0.0.
assert np.finfo(np.longdouble).nmant >= 63, "the FP64 bound's reference needs a long double of at least 64 bits of mantissa"
U64 = 2.0 ** -53


def seg_sum_ld(idx, w, n):
    """Per-slot sums of the long-double weights w: out[k] = sum of w[idx == k], k in [0, n).  (np.bincount would
    cast the weights to double.)"""
    w = np.asarray(w, np.longdouble)
    out = np.zeros(n, np.longdouble)
    if len(idx) == 0:
        return out
    order = np.argsort(idx, kind="stable")
    si = np.asarray(idx)[order]
    slots, starts = np.unique(si, return_index=True)
    out[slots] = np.add.reduceat(w[order], starts)
    return out


def _exact_sums(idx, x, y, n):
    """(sum, count, absolute sum) per slot of the products x * y, formed and summed in long double."""
    w = np.asarray(x, np.longdouble) * np.asarray(y, np.longdouble)
    return seg_sum_ld(idx, w, n), np.bincount(idx, minlength=n).astype(np.int64), seg_sum_ld(idx, np.abs(w), n)


def exact_forward(A, B, Cp, Ci, av, bv):
    """(ref_ld, m, S) of A*B with the values (av, bv) on the pattern (Cp, Ci), which may be a mask: per entry
    the long-double sum of its kept products, their count and the sum of their absolute values."""
    p, q, s = expand(A.ptr, A.col, B.ptr, B.col, Cp, Ci, B.N)
    return _exact_sums(s, av[p], bv[q], len(Ci))


def exact_grad(pqs, av, bv, G, nnzA, nnzB):
    """The (ref_ld, m, S) triples of dA and of dB for the cotangent G over the kept products pqs."""
    p, q, s = pqs
    return _exact_sums(p, bv[q], G[s], nnzA), _exact_sums(q, av[p], G[s], nnzB)


def assert_f64_bound(got, ref_ld, m, S, what):
    """got (float64) against the long-double reference within 1.01 m 2^-53 S; m = 0: exactly 0.0; no NaN.
    Prints and returns the worst err / bound (0.0 where every entry is exact)."""
    got = np.asarray(got)
    assert got.dtype == np.float64 and got.shape == ref_ld.shape == m.shape == S.shape, f"{what}: shape"
    assert not np.isnan(got).any(), f"{what}: every entry is written"
    assert np.all(got[m == 0] == 0.0), f"{what}: entries no kept product reaches are exactly 0.0"
    assert m.max(initial=0) < 2 ** 20
    err = np.abs(got.astype(np.longdouble) - ref_ld)
    bound = np.longdouble(1.01 * U64) * m.astype(np.longdouble) * S
    ratio = np.zeros(len(got), np.longdouble)
    np.divide(err, bound, out=ratio, where=bound > 0)
    worst = float(ratio.max(initial=0.0))
    print(f"f64 bound, {what}: worst err / bound {worst:.3f} over {len(got)} entries, max m {m.max(initial=0)}")
    bad = err > bound
    assert not bad.any(), f"{what}: {bad.sum()} of {len(got)} entries outside 1.01 m 2^-53 S (worst err / bound {worst:.3e})"
    return worst


def wide_values(n, seed):
    """uniform(0.5, 1) * 2^k, k an integer of [-20, 20], with a random sign: full 53-bit mantissas over 41 binades.
    Magnitudes lie in [2^-21, 2^20) and products of two in [2^-42, 2^40): nothing is subnormal, nothing overflows."""
    rng = np.random.default_rng(seed)
    return np.ldexp(rng.uniform(0.5, 1.0, n), rng.integers(-20, 21, n)) * rng.choice([-1.0, 1.0], n)


# ------------------------------------------- IEEE propagation of Inf, NaN and stored zeros ---
# The contract of every value path for non-finite inputs (include/mhspgemm.h), free of any summation order: an
# output entry forms every kept product x * y and nothing else.  With each product classified in IEEE double
# (0 * Inf and anything times NaN are NaN), the entry is NaN if a product is NaN or both +Inf and -Inf products
# occur, +Inf or -Inf if only that sign of infinity occurs, and otherwise finite within the rounding bound of
# its products, 1.01 m u S (exactly 0.0 where m = 0).  A stored zero is an ordinary entry.  Finite magnitudes
# stay in the suite's ranges (wide_values; [0.1, 1) for FP32), so no finite partial sum overflows and the class
# of an entry does not depend on the order.
FINITE, POS_INF, NEG_INF, IS_NAN = 0, 1, 2, 3
CLASS_NAMES = ("finite", "+Inf", "-Inf", "NaN")
U32 = 2.0 ** -24


def inject_nonfinite(v, seed, rate=0.004, least=6, zeros=True):
    """A copy of v with k = max(least, int(rate * n)) entries, drawn without replacement, set to +Inf, -Inf, NaN
    and 0.0 in turn (zeros=False: the first three)."""
    out = np.array(v, copy=True)
    n = len(out)
    k = max(least, int(rate * n))
    pos = np.random.default_rng(seed).choice(n, k, replace=False)
    marks = np.array([np.inf, -np.inf, np.nan, 0.0] if zeros else [np.inf, -np.inf, np.nan], out.dtype)
    out[pos] = marks[np.arange(k) % len(marks)]
    return out


def classes_of(v):
    """The class of every value: FINITE, POS_INF, NEG_INF or IS_NAN."""
    v = np.asarray(v, np.float64)
    return np.where(np.isnan(v), IS_NAN, np.where(v == np.inf, POS_INF, np.where(v == -np.inf, NEG_INF, FINITE))).astype(np.int8)


def product_classes(idx, x, y, n):
    """The class of each slot k of [0, n) from the products x[i] * y[i] with idx[i] == k, formed in IEEE double."""
    with np.errstate(invalid="ignore", over="ignore"):
        w = np.asarray(x, np.float64) * np.asarray(y, np.float64)
    idx = np.asarray(idx, np.int64)
    nan = np.bincount(idx[np.isnan(w)], minlength=n) > 0
    pos = np.bincount(idx[w == np.inf], minlength=n) > 0
    neg = np.bincount(idx[w == -np.inf], minlength=n) > 0
    return np.where(nan | (pos & neg), IS_NAN, np.where(pos, POS_INF, np.where(neg, NEG_INF, FINITE))).astype(np.int8)


def class_counts(cls):
    return {CLASS_NAMES[c]: int(np.count_nonzero(cls == c)) for c in range(4)}


def nonfinite_reference(idx, x, y, n, u):
    """What the contract above asks of an output of n entries for the kept products x[i] * y[i] of slot idx[i]:
    (classes, ref, m, S, u) -- the class per entry, and for the finite entries, in their order, the sum of their
    products (all of them finite), their count and their absolute sum.  u = 2^-53: long-double sums; u = 2^-24:
    double sums on the inputs as given, which the caller has rounded to float32.  Computed once and read only."""
    assert u in (U64, U32), u
    idx = np.asarray(idx, np.int64)
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    want = product_classes(idx, x, y, n)
    fin = want == FINITE
    keep = fin[idx]  # the products of the finite entries: every one of them finite
    slot = (np.cumsum(fin) - 1)[idx[keep]]
    nf = int(fin.sum())
    m = np.bincount(slot, minlength=nf).astype(np.int64)
    assert m.max(initial=0) < (2 ** 20 if u == U64 else 2 ** 16)
    if u == U64:
        ref, _, S = _exact_sums(slot, x[keep], y[keep], nf)
    else:
        w = x[keep] * y[keep]
        ref, S = np.bincount(slot, w, nf), np.bincount(slot, np.abs(w), nf)
    assert np.isfinite(S.astype(np.float64)).all()
    return want, ref, m, S, u


def assert_nonfinite_reference(got, reference, what, only=None):
    """got against a nonfinite_reference: the classes equal entry for entry, the finite entries within 1.01 m u S of
    their sums, and exactly 0.0 where m = 0.  only (a boolean mask): the entries judged.  Returns the classes."""
    want, ref, m, S, u = reference
    got = np.asarray(got).astype(np.float64)
    n = len(want)
    assert got.shape == (n,), f"{what}: shape"
    only = np.ones(n, bool) if only is None else np.asarray(only, bool)
    have = classes_of(got)
    wrong = (want != have) & only
    if wrong.any():
        pairs = {f"{CLASS_NAMES[a]} -> {CLASS_NAMES[b]}": int(np.count_nonzero(wrong & (want == a) & (have == b)))
                 for a in range(4) for b in range(4) if a != b}
        pairs = {k: c for k, c in pairs.items() if c}
        raise AssertionError(f"{what}: {wrong.sum()} of {only.sum()} entries in another class than their products' "
                             f"(contract -> got: {pairs}; first at entry {int(np.nonzero(wrong)[0][0])})")
    fin = want == FINITE
    g, judged = got[fin], only[fin]
    assert np.all(g[(m == 0) & judged] == 0.0), f"{what}: entries no kept product reaches are exactly 0.0"
    if u == U64:
        err = np.abs(g.astype(np.longdouble) - ref)
        bound = np.longdouble(1.01 * U64) * m.astype(np.longdouble) * S
    else:
        err, bound = np.abs(g - ref), 1.01 * U32 * m * S
    ratio = np.zeros(len(g), err.dtype)
    np.divide(err, bound, out=ratio, where=(bound > 0) & judged)
    worst = float(ratio.max(initial=0.0))
    print(f"non-finite contract, {what}: {class_counts(want[only])}, worst err / bound {worst:.3f} on the finite "
          f"entries, max m {m.max(initial=0)}")
    bad = (err > bound) & judged
    assert not bad.any(), (f"{what}: {bad.sum()} of {judged.sum()} finite entries outside 1.01 m u S, "
                           f"u = 2^{int(np.log2(u))} (worst err / bound {worst:.3e})")
    return want


def assert_nonfinite_contract(got, idx, x, y, n, u, what):
    """The whole check of an output against the contract above: nonfinite_reference, then assert_nonfinite_reference."""
    return assert_nonfinite_reference(got, nonfinite_reference(idx, x, y, n, u), what)


# ------------------------------------------------------------ the edge ladder ---
# Rows that sit exactly on a bin or class edge of csrc/mhs_shape.hpp / mhs_valplan.hpp.  The edges themselves
# come from tests/golden/shape_edges.json (printed by tests/shape_edges.cpp from the headers); the families
# below build a matrix pair whose first EDGE_COPIES * R rows of A all have the prescribed parameters.  Every
# value is an integer of +-{1, 2, 3}: products and partial sums stay integers below 9 * flop < 2^53, so the
# product is exact in any summation order and the tests compare with np.array_equal.
EDGE_COPIES = 8  # two blocks of four waves: every wave of a block holds an edge row at once


def load_edges():
    return json.loads((GOLDEN / "shape_edges.json").read_text())


def edge_values(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.integers(1, 4, n) * rng.choice([-1, 1], n)).astype(np.float64)


def _edge_pair(M, K, N, alen, acol, blen, bcol, seed):
    Ap = np.zeros(M + 1, np.int64)
    np.cumsum(alen, out=Ap[1:])
    Bp = np.zeros(K + 1, np.int64)
    np.cumsum(blen, out=Bp[1:])
    assert Ap[-1] == len(acol) and Bp[-1] == len(bcol) and N < 2**31 and Ap[-1] < 2**31 and Bp[-1] < 2**31
    acol, bcol = np.asarray(acol, np.int32), np.asarray(bcol, np.int32)
    return ((M, K, Ap.astype(np.int32), acol, edge_values(len(acol), seed)),
            (K, N, Bp.astype(np.int32), bcol, edge_values(len(bcol), seed + 1)))


def _ragged(lens):
    """Index within its row of every entry of rows of the given lengths."""
    lens = np.asarray(lens, np.int64)
    return np.arange(lens.sum()) - np.repeat(np.cumsum(lens) - lens, lens)


def edge_band(s, n, stride=1, R=1, copies=EDGE_COPIES, seed=1):
    """band(s, n): B row k holds c[k % s] columns at the start of tile stride * k, c spreading n over s tiles
    (at most 64 a tile); A row j is the s consecutive B rows from j, R times in a row (R > 1: a row group).
    Every row has tile span stride * (s - 1) + 1, t = s tiles, n C entries, n products, s tile products and
    s A entries; c is periodic, so the copies differ in pattern only.  stride 1 is direct mode; a wider
    stride is scatter(t, n, stride), hash mode."""
    assert s <= n <= 64 * s
    c = n // s + (np.arange(s) < n % s)
    K = s + copies - 1
    blen = c[np.arange(K) % s]
    bcol = np.repeat(64 * stride * np.arange(K, dtype=np.int64), blen) + _ragged(blen)
    first = np.repeat(np.arange(copies), R)
    acol = (first[:, None] + np.arange(s)[None, :]).reshape(-1)
    return _edge_pair(copies * R, K, 64 * stride * K, np.full(copies * R, s), acol, blen, bcol, seed)


def edge_scatter(t, n, stride, copies=EDGE_COPIES, seed=1):
    return edge_band(t, n, stride=stride, copies=copies, seed=seed)


def edge_work(flop, copies=EDGE_COPIES, seed=1):
    """work(flop): A row j repeats the full 64-column B row j flop // 64 times; B row copies + j adds the
    remainder in the same tile.  n = 64 over one tile (528 bytes of tables) whatever the product count."""
    q, r = divmod(flop, 64)
    assert q >= 1
    blen = np.concatenate([np.full(copies, 64), np.full(copies, r)])
    bcol = np.repeat(64 * (np.arange(2 * copies, dtype=np.int64) % copies), blen) + _ragged(blen)
    alen = np.full(copies, q + (r > 0))
    acol = np.repeat(np.arange(copies), alen)
    if r:
        acol[np.cumsum(alen) - 1] = copies + np.arange(copies)
    return _edge_pair(copies, 2 * copies, 64 * copies, alen, acol, blen, bcol, seed)


def edge_symwork(tflop, copies=EDGE_COPIES, seed=1):
    """One-entry B rows: A row j repeats B row j (one column, in tile j) tflop times -- tile work without a table."""
    acol = np.repeat(np.arange(copies), tflop)
    return _edge_pair(copies, copies, 64 * copies, np.full(copies, tflop), acol, np.ones(copies, np.int64),
                      64 * np.arange(copies, dtype=np.int64), seed)


def edge_val(n, span, products, copies=EDGE_COPIES, seed=1):
    """A C row of n entries over a column span of `span` with `products` products: B row 3j holds the row's
    first n - 1 columns, row 3j + 2 its last one, row 3j + 1 the first (products - 1) % (n - 1) columns again;
    A row j repeats row 3j (products - 1) // (n - 1) times, then the other two.  Copy j starts at column 100 j."""
    assert 2 <= n <= span and products >= n
    m, r = divmod(products - 1, n - 1)
    blen = np.tile([n - 1, r, 1], copies)
    base = np.repeat(100 * np.arange(copies, dtype=np.int64), 3)
    bcol = np.repeat(base, blen) + _ragged(blen)
    bcol[np.cumsum(blen)[2::3] - 1] += span - 1
    one = np.concatenate([np.zeros(m, np.int64), np.ones(1 if r else 0, np.int64), np.full(1, 2)])
    acol = (3 * np.arange(copies)[:, None] + one[None, :]).reshape(-1)
    return _edge_pair(copies, 3 * copies, 100 * copies + span, np.full(copies, len(one)), acol, blen, bcol, seed)


def edge_rows(M, s=201, seed=1):
    """M rows for the row-count edges: A bidiagonal (row i: B rows i, i + 1) with a few band rows of s B rows
    mixed in (first rows, the middle, the last row); B row k holds 1, 2, 3, 1, ... columns at the start of tile k."""
    K = M + s
    blen = 1 + np.arange(K) % 3
    bcol = np.repeat(64 * np.arange(K, dtype=np.int64), blen) + _ragged(blen)
    alen = np.full(M, 2)
    alen[[0, min(5, M - 1), M // 2, M - 1]] = s
    acol = np.repeat(np.arange(M, dtype=np.int64), alen) + _ragged(alen)
    return _edge_pair(M, K, 64 * K, alen, acol, blen, bcol, seed)


def edge_case(family, params, R=1):
    """The matrix pair of one side of a rung of shape_edges.json."""
    if family == "band":
        return edge_band(params["s"], params["n"], R=R)
    if family == "scatter":
        return edge_scatter(params["t"], params["n"], params["stride"])
    if family == "work":
        return edge_work(params["flop"])
    if family == "symwork":
        return edge_symwork(params["tflop"])
    if family == "val":
        return edge_val(params["n"], params["span"], params["products"])
    raise ValueError(family)


def _per_row(ptr, per_entry):
    """Sum of an integer per-entry quantity over each CSR row (exact: cumulative sums in int64)."""
    cs = np.zeros(len(per_entry) + 1, np.int64)
    np.cumsum(per_entry, out=cs[1:])
    return cs[ptr[1:]] - cs[ptr[:-1]]


def _new_tile(ptr, col):
    """1 where an entry opens a new 64-column tile of its row."""
    tile = col.astype(np.int64) >> 6
    new = np.ones(len(col), np.int64)
    new[1:] = tile[1:] != tile[:-1]
    new[ptr[:-1][np.diff(ptr) > 0]] = 1
    return new


def row_shapes(A, B, Cp, Ci):
    """What the bin ladders see of every row of C = A*B, recomputed from the matrices and the oracle's pattern:
    a dict of int64 arrays span (tiles from the first to the last), t (distinct tiles), n (C entries), flop
    (products), tflop (B tiles walked), nA (A entries), and colspan (last column - first + 1)."""
    _, _, Ap, Ac, _ = A
    _, _, Bp, Bc, _ = B
    Ap, Bp, Cp = Ap.astype(np.int64), Bp.astype(np.int64), np.asarray(Cp, np.int64)
    btiles = _per_row(Bp, _new_tile(Bp, Bc))
    n = np.diff(Cp)
    has = n > 0
    first, last = Cp[:-1][has], Cp[1:][has] - 1
    span, colspan = np.zeros(len(n), np.int64), np.zeros(len(n), np.int64)
    span[has] = (Ci[last].astype(np.int64) >> 6) - (Ci[first].astype(np.int64) >> 6) + 1
    colspan[has] = Ci[last].astype(np.int64) - Ci[first] + 1
    return {"span": span, "t": _per_row(Cp, _new_tile(Cp, Ci)), "n": n, "flop": _per_row(Ap, np.diff(Bp)[Ac]),
            "tflop": _per_row(Ap, btiles[Ac]), "nA": np.diff(Ap), "colspan": colspan}


@functools.lru_cache(maxsize=None)
def many_a_entries():
    """A with rows of 65 to 700 entries over tiny_zoo's B, the product's pattern and its kept products (expand):
    wave rows whose A entries need more than one stage (64 entries a stage, 256 in a block), and a block's row."""
    import mhspgemm
    from oracle import oracle as orc
    (_, K, _, _, _), Bt = tiny_zoo(7)
    _, N, Bp, Bc, Bv = Bt
    rng = np.random.default_rng(23)
    blen = np.diff(Bp)
    narrow = np.nonzero((np.arange(K) % 5 == 1))[0]               # B rows inside columns [0, 200): a direct span
    wide = np.nonzero((np.arange(K) % 5 >= 2) & (blen > 0))[0]    # B rows anywhere in [0, 5000): searched
    arows = []
    for na in (65, 100, 150, 257, 300):
        arows.append(np.sort(rng.choice(narrow, na, replace=False)))
        arows.append(np.sort(rng.choice(wide, na, replace=False)))
    arows.append(np.sort(rng.choice(wide, 700, replace=False)))    # past the wave's product cap: a block's row
    Ap = np.zeros(len(arows) + 1, np.int64)
    Ap[1:] = np.cumsum([len(r) for r in arows])
    Ac = np.concatenate(arows).astype(np.int32)
    A = mhspgemm.CSR(len(arows), K, Ap.astype(np.int32), Ac, np.ones(len(Ac)))
    B = csr_of(Bt)
    Cp, Ci, _ = orc.spgemm(A.ptr, A.col, A.val, B.ptr, B.col, B.val, B.N)
    return A, B, Cp, Ci, expand(A.ptr, A.col, B.ptr, B.col, Cp, Ci, B.N)
