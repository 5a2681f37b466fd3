"""Repeated column indices in CSR rows, placed where the kernels' paths depend on them (test infrastructure).

include/mhspgemm.h: "B's column indices are sorted ascending within each row" (non-strict: ERR_UNSORTED is raised
on c < pc only) and "duplicates in A or B are summed".  with_repeats turns a matrix with strictly ascending rows
into its repeat twin -- the same rows, the same distinct columns, some entries stored several times --
merge_repeats sums a twin's repeats back into one entry each, and repeat_kinds says which kinds of repeat a
matrix holds, from the matrix alone.  The kinds:

  a  an adjacent pair and a triple in mid-row
  b  the row's first entry repeated; the row's last entry repeated
  c  one column on the row positions 63 and 64 -- the edge of a mask-formation chunk of every lane-group width
     (8, 16, 32, 64) -- and one on the positions 31 and 32 (k_mask_lane's MASK_LANE_LONG)
  d  repeats on both sides of a tile edge: the last entry of one 64-column tile and the first of the next, both
     repeated (d_exact: the columns 64 t + 63 and 64 t + 64 themselves)
  e  one column r times, r = 2, 65, 200: a tile run longer than a wave.  In a row of one entry (e_single) the
     run has one bit; where a matrix has no such row the 65 and the 200 go to one entry of a longer row (e_inrow)
  f  a whole row doubled, every entry twice
  g  two adjacent rows with the same distinct columns and the same multiplicities: a same-pattern run
  h  two adjacent rows with the same distinct columns and the same length but other multiplicities
     ([a, a, b] / [a, b, b]): not a run
  i  a random remainder: a share of the entries of the rows no other kind took, 2 or 3 times.  Adjacent rows with
     one pattern mostly draw once for all of them (runs that live on, kind g), sometimes anew (broken runs)

g and h need two adjacent rows with one pattern in the input, and the twin keeps the input's distinct pattern:
can_hold says which kinds an input can take.

Values are integers of +-{1, 2, 3} (tests/_util.py's edge_values): every sum of products is an integer, exact in
double in any order, and in float while 9 * (products of an entry) < 2^24 (max_products).  The repeats of one
entry get pairwise different magnitudes where there are at most three of them and a random cycle of the three
magnitudes past that (there are only three): a repeat used twice and its neighbour never changes the sum."""
from __future__ import annotations

import functools

import numpy as np

KINDS = "abcdefghi"
RUNS = (2, 65, 200)
_PERMS = np.array([[1, 2, 3], [1, 3, 2], [2, 1, 3], [2, 3, 1], [3, 1, 2], [3, 2, 1]], np.float64)


def _ragged(lens):
    lens = np.asarray(lens, np.int64)
    return np.arange(lens.sum()) - np.repeat(np.cumsum(lens) - lens, lens)


def _ptr(lens):
    p = np.zeros(len(lens) + 1, np.int64)
    np.cumsum(lens, out=p[1:])
    assert p[-1] < 2 ** 31
    return p.astype(np.int32)


def is_legal(Bt):
    """Rows ascending (non-strict) and columns in [0, N)."""
    K, N, ptr, col, val = Bt
    if len(ptr) != K + 1 or ptr[0] != 0 or ptr[-1] != len(col) or len(val) != len(col) or np.any(np.diff(ptr) < 0):
        return False
    if len(col) == 0:
        return True
    rows = np.repeat(np.arange(K), np.diff(ptr))
    down = (col[1:] < col[:-1]) & (rows[1:] == rows[:-1])
    return bool(col.min() >= 0 and col.max() < N and not down.any())


def split_repeats(Bt):
    """(ptr, col, mult, start) of the distinct entries of a matrix with ascending rows: the merged pattern, how
    often each of its entries is stored, and where its first copy sits in Bt's arrays."""
    K, N, ptr, col, val = Bt
    rows = np.repeat(np.arange(K), np.diff(ptr))
    new = np.ones(len(col), bool)
    new[1:] = (col[1:] != col[:-1]) | (rows[1:] != rows[:-1])
    start = np.nonzero(new)[0]
    mult = np.diff(np.append(start, len(col)))
    return _ptr(np.bincount(rows[new], minlength=K)), col[new].astype(np.int32), mult.astype(np.int64), start


def merge_repeats(Bt):
    """The same matrix with each row's repeats summed into one entry: rows strictly ascending."""
    K, N, ptr, col, val = Bt
    p1, c1, mult, start = split_repeats(Bt)
    v1 = np.add.reduceat(np.asarray(val, np.float64), start) if len(col) else np.zeros(0)
    return K, N, p1, c1, v1


def _same_as_previous(ptr, col):
    """same[k]: row k is not empty and has the columns of row k - 1."""
    K = len(ptr) - 1
    same = np.zeros(K, bool)
    for k in range(1, K):
        a, b, c = ptr[k - 1], ptr[k], ptr[k + 1]
        same[k] = c > b and c - b == b - a and np.array_equal(col[a:b], col[b:c])
    return same


def can_hold(Bt):
    """The kinds a twin of this strictly ascending matrix can hold."""
    K, N, ptr, col, val = Bt
    L = np.diff(ptr)
    tile = col.astype(np.int64) >> 6
    rows = np.repeat(np.arange(K), L)
    edge = (rows[1:] == rows[:-1]) & (tile[1:] != tile[:-1])
    same = _same_as_previous(ptr, col)
    pairs = np.count_nonzero(same & (L >= 2))
    can = {"a": (L >= 5).any(), "b": (L >= 2).any(), "c": (L >= 2).any(), "d": edge.any(), "e": (L >= 1).any(),
           "f": (L >= 2).any(), "g": pairs >= 2, "h": pairs >= 1, "i": (L >= 1).any()}
    return {k for k in KINDS if can[k]}


def repeat_kinds(Bt):
    """Counts of every kind of repeat in a matrix with ascending rows, from the matrix alone."""
    K, N, ptr, col, val = Bt
    p1, c1, mult, start = split_repeats(Bt)
    L1 = np.diff(p1).astype(np.int64)
    rows = np.repeat(np.arange(K), L1)
    at = _ragged(L1)
    Lr = L1[rows]
    first, last = at == 0, at == Lr - 1
    pos = start - np.asarray(ptr, np.int64)[rows]  # the row position of an entry's first copy
    c = {}
    mid = ~first & ~last
    c["a_pair"] = int(np.count_nonzero(mid & (mult == 2)))
    c["a_triple"] = int(np.count_nonzero(mid & (mult == 3)))
    c["b_first"] = int(np.count_nonzero(first & (mult >= 2) & (Lr >= 2)))
    c["b_last"] = int(np.count_nonzero(last & (mult >= 2) & (Lr >= 2)))
    for P in (63, 31):
        c[f"c{P}"] = int(np.count_nonzero((pos <= P) & (pos + mult - 1 >= P + 1)))
    tile = c1.astype(np.int64) >> 6
    both = (rows[1:] == rows[:-1]) & (tile[1:] != tile[:-1]) & (mult[1:] >= 2) & (mult[:-1] >= 2)
    c["d"] = int(np.count_nonzero(both))
    c["d_exact"] = int(np.count_nonzero(both & (c1[:-1] % 64 == 63) & (c1[1:] == c1[:-1] + 1)))
    for r in RUNS:
        c[f"e_single_{r}"] = int(np.count_nonzero((Lr == 1) & (mult == r)))
        c[f"e_inrow_{r}"] = int(np.count_nonzero((Lr > 1) & (mult == r))) if r > 3 else 0
    two = np.zeros(K, bool)
    has = L1 > 0
    if has.any():
        lo = np.minimum.reduceat(mult, p1[:-1][has])
        hi = np.maximum.reduceat(mult, p1[:-1][has])
        two[has] = (lo == 2) & (hi == 2)
    c["f"] = int(np.count_nonzero(two & (L1 >= 2)))
    g = h = 0
    same = _same_as_previous(p1, c1)
    for k in np.nonzero(same)[0]:
        ma, mb = mult[p1[k - 1]:p1[k]], mult[p1[k]:p1[k + 1]]
        if np.array_equal(ma, mb):
            g += int(ma.max() > 1)
        elif ma.sum() == mb.sum():
            h += 1
    c["g"], c["h"] = g, h
    c["repeated_entries"] = int(np.count_nonzero(mult > 1))
    c["longest_tile_run"] = int(_longest_tile_run(ptr, col))
    return c


def _longest_tile_run(ptr, col):
    """The most stored entries any row holds in one 64-column tile."""
    if len(col) == 0:
        return 0
    rows = np.repeat(np.arange(len(ptr) - 1, dtype=np.int64), np.diff(ptr))
    key = rows * (1 << 26) + (col.astype(np.int64) >> 6)
    new = np.ones(len(key), bool)
    new[1:] = key[1:] != key[:-1]
    s = np.nonzero(new)[0]
    return np.diff(np.append(s, len(key))).max()


def present(counts):
    """The kinds a..h whose every part occurs (i: counts["i"], which with_repeats adds)."""
    c = counts
    p = set()
    if c["a_pair"] and c["a_triple"]:
        p.add("a")
    if c["b_first"] and c["b_last"]:
        p.add("b")
    if c["c63"] and c["c31"]:
        p.add("c")
    if c["d"]:
        p.add("d")
    if all(c[f"e_single_{r}"] + c[f"e_inrow_{r}"] for r in RUNS if r > 3):
        p.add("e")
    for k in "fgh":
        if c[k]:
            p.add(k)
    if c.get("i", 0):
        p.add("i")
    return p


def with_repeats(Bt, seed, share=0.1, kinds=KINDS, runs=RUNS, per_kind=2, group=1, inflate=True, follow=0.75):
    """The repeat twin of (K, N, ptr, col, val), rows strictly ascending: (twin, counts).  Each kind of `kinds` goes
    to per_kind rows that are long enough for it and that no other kind took (kind e: a row of one entry per r of
    `runs`, else one entry of a longer row for the r past 3), and a share `share` of the entries of the remaining rows
    is stored 2 or 3 times (kind i).  inflate: where no row reaches the positions 63 / 64 (31 / 32), kind c repeats
    one entry of a shorter row until it lies on both.  group = R > 1: rows k R + 1 .. k R + R - 1 that have the
    columns of row k R take its multiplicities (the dof rows of a FEM node stay identical; no g / h placement: g
    comes with the groups, h would break them).  counts: repeat_kinds of the twin, and "i"."""
    K, N, ptr, col, val = Bt
    ptr = np.asarray(ptr, np.int64)
    L = np.diff(ptr)
    rows = np.repeat(np.arange(K), L)
    assert len(col) == 0 or not ((col[1:] <= col[:-1]) & (rows[1:] == rows[:-1])).any(), "the input's rows ascend strictly"
    rng = np.random.default_rng(seed)
    mult = np.ones(len(col), np.int64)
    same = _same_as_previous(ptr, col)
    follower = np.zeros(K, bool)
    lead = np.arange(K)
    if group > 1:
        for k in range(K):
            h = k - k % group
            if h != k and L[k] == L[h] and L[k] > 0 and np.array_equal(col[ptr[k]:ptr[k + 1]], col[ptr[h]:ptr[h + 1]]):
                follower[k], lead[k] = True, h
    free = ~follower & (L > 0)

    def take(cond, n=per_kind):
        cand = np.nonzero(free & cond)[0]
        got = rng.choice(cand, min(n, len(cand)), replace=False) if len(cand) else cand
        free[got] = False
        return [int(k) for k in got]

    tile = col.astype(np.int64) >> 6
    if "e" in kinds:
        for r in sorted(runs, reverse=True):
            for k in take(L == 1, 1):
                mult[ptr[k]] = r
    if group == 1 and ("g" in kinds or "h" in kinds):
        for want in ("h", "g"):
            if want not in kinds:
                continue
            for _ in range(per_kind):
                cand = np.nonzero(same & (L >= 2) & free & np.roll(free, 1))[0]
                if not len(cand):
                    break
                k = int(rng.choice(cand))
                free[[k - 1, k]] = False
                j = int(rng.integers(0, L[k] - 1))
                mult[ptr[k - 1] + j] = 2
                mult[ptr[k] + (j if want == "g" else j + 1)] = 2
    if "d" in kinds:
        edge = np.zeros(len(col), bool)
        edge[:-1] = (rows[1:] == rows[:-1]) & (tile[1:] != tile[:-1])
        exact = edge.copy()
        exact[:-1] &= (col[:-1] % 64 == 63) & (col[1:] == col[:-1] + 1)
        for which in (exact, edge):
            has = np.zeros(K, bool)
            has[rows[which]] = True
            for k in take(has, 1 if which is exact else per_kind):
                j = int(rng.choice(np.nonzero(which[ptr[k]:ptr[k + 1]])[0]))
                mult[ptr[k] + j] = 2
                mult[ptr[k] + j + 1] = 2 + (which is edge)
    if "c" in kinds:
        for P in (63, 31):
            got = take(L > P + 1)
            for k in got:
                mult[ptr[k] + P] = 2
            if inflate:  # one entry of a shorter row stored until it covers both positions (mid-row, and the last)
                for k, j in zip(take((L >= 3) & (L <= P)), (1, -1)):
                    j = j % L[k]
                    mult[ptr[k] + j] = P + 2 - j
    if "f" in kinds:
        for k in take(L >= 2):
            mult[ptr[k]:ptr[k + 1]] = 2
    if "a" in kinds:
        for k in take(L >= 5):
            mult[ptr[k] + L[k] // 3] = 2
            mult[ptr[k] + 2 * L[k] // 3] = 3
    if "b" in kinds:
        for k in take(L >= 2):
            mult[ptr[k]] = 2
            mult[ptr[k + 1] - 1] = 3
    if "e" in kinds:  # the long runs no one-entry row took: one mid entry of a longer row each
        for r in runs:
            if r > 3 and not np.any(mult[ptr[:-1][L == 1]] == r):
                for k in take(L >= 3, 1):
                    mult[ptr[k] + L[k] // 2] = r
    n_i = 0
    if "i" in kinds:
        drawn = np.zeros(K, bool)
        for k in np.nonzero(free)[0]:
            a, b = ptr[k], ptr[k + 1]
            if group == 1 and same[k] and drawn[k - 1] and rng.random() < follow:
                mult[a:b] = mult[ptr[k - 1]:a]
            else:
                hit = rng.random(b - a) < share
                mult[a:b] = np.where(hit, rng.integers(2, 4, b - a), 1)
            drawn[k] = True
            n_i += int(np.count_nonzero(mult[a:b] > 1))
    for k in np.nonzero(follower)[0]:
        h = lead[k]
        mult[ptr[k]:ptr[k + 1]] = mult[ptr[h]:ptr[h + 1]]
    col2 = np.repeat(col, mult).astype(np.int32)
    perm = np.repeat(rng.integers(0, 6, len(col)), mult)
    val2 = _PERMS[perm, _ragged(mult) % 3] * rng.choice([-1.0, 1.0], len(col2))
    cs = np.zeros(len(col) + 1, np.int64)
    np.cumsum(mult, out=cs[1:])
    twin = (K, N, _ptr(cs[ptr[1:]] - cs[ptr[:-1]]), col2, val2)
    counts = repeat_kinds(twin)
    counts["i"] = n_i
    return twin, counts


def magnitudes_differ(Bt):
    """Within every run of at most three copies of one entry the magnitudes are pairwise different, and in longer
    runs neighbours differ."""
    K, N, ptr, col, val = Bt
    if len(col) < 2:
        return True
    rows = np.repeat(np.arange(K), np.diff(ptr))
    mag = np.abs(val)
    eq1 = (col[1:] == col[:-1]) & (rows[1:] == rows[:-1])
    eq2 = (col[2:] == col[:-2]) & (rows[2:] == rows[:-2])
    return bool(not (eq1 & (mag[1:] == mag[:-1])).any() and not (eq2 & (mag[2:] == mag[:-2])).any())


def integer_values(v):
    v = np.asarray(v)
    return bool(np.all(np.isin(np.abs(v), (1.0, 2.0, 3.0))))


def max_products(s, n):
    """The most products any of n output entries sums, s the slot of every product (tests/_util.py's expand)."""
    return int(np.bincount(s, minlength=n).max(initial=0))


# ------------------------------------------------------------------ the operands of the repeat tests ---
ZOO_NAMES = ("bin_zoo", "tiny_zoo", "run_zoo", "group_zoo", "near_zoo")
NUM_WS_WORK = 8192  # mhs_shape.hpp: the products a row of the small wave bins (grouped ones included) may have
# The aliased cases (A * A, A itself the twin): the operand, the variant, with_repeats' arguments.
# uniform: the three dof rows of a node take the same multiplicities at the same positions (group=3), so the rows of
# a node stay identical, multiplicities included, and the row groups of the clean matrix stay row groups -- the exact
# census of fem_capped_group_grid (325 groups, one per node of the 5 x 5 x 13 grid) holds.  Kinds e and f and the
# inflated c are left out there, and the share is small: a row of 65 or 200 more entries, or a doubled one, has more
# than NUM_WS_WORK products and leaves the grouped bin (tests/test_b_repeats_host.py holds every row of these twins to that limit).  g comes
# with the groups; h would break them.
# ragged: every row draws for itself (group=1), so the rows of a node differ in their multiplicities -- or, in
# perturbed_fem, in a few entries as well: near row groups.
ALIASED = {
    "fem_5_5_13": ("fem_5_5_13", dict(share=0.02, kinds="abcdi", group=3, inflate=False)),
    "fem_5_4_9": ("fem_5_4_9", dict(share=0.02, kinds="abcdi", group=3, inflate=False)),
    "perturbed_fem": ("perturbed_fem", dict(share=0.02, follow=0.0)),
    "fem_5_5_13_ragged": ("fem_5_5_13", dict(share=0.02, follow=0.0)),
}
UNIFORM = ("fem_5_5_13", "fem_5_4_9")


def _base(name):
    from mhspgemm import synth
    from _util import bin_zoo, group_zoo, near_zoo, run_zoo, tiny_zoo
    if name == "fem_5_5_13":
        F = synth.fem_grid(5, 5, 13, 3, seed=5)
    elif name == "fem_5_4_9":
        F = synth.fem_grid(5, 4, 9, dof=3)
    elif name == "perturbed_fem":
        from test_gpu_parity import _perturbed_fem
        F = _perturbed_fem(7, 6, 24, 0.03, seed=31)
    else:
        return {"bin_zoo": bin_zoo, "tiny_zoo": lambda: tiny_zoo(7), "run_zoo": lambda: run_zoo(5),
                "group_zoo": lambda: group_zoo(3), "near_zoo": near_zoo}[name]()
    return (F.M, F.N, F.ptr, F.col, F.val), None


@functools.lru_cache(maxsize=None)
def twin_operands(name):
    """(At, Bt, counts, base) of a case: a zoo's A with integer values and the repeat twin of its B, or for the ALIASED
    names the twin of the square matrix and Bt None (B is A).  base: the matrix the twin was made from.  Read only."""
    from _util import edge_values
    if name in ALIASED:
        base, _ = _base(ALIASED[name][0])
        twin, counts = with_repeats(base, 7, **ALIASED[name][1])
        return twin, None, counts, base
    At, Bt = _base(name)
    twin, counts = with_repeats(Bt, 7)
    return (*At[:4], edge_values(len(At[3]), 70)), twin, counts, Bt


def row_products(At, Bt):
    """Products of every row of A * B."""
    Ap, Ac, Bp = np.asarray(At[2], np.int64), At[3], np.asarray(Bt[2], np.int64)
    cs = np.zeros(len(Ac) + 1, np.int64)
    np.cumsum(np.diff(Bp)[Ac], out=cs[1:])
    return cs[Ap[1:]] - cs[Ap[:-1]]
