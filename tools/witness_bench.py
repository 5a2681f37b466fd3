#!/usr/bin/env python3
"""witness_bench.py -- the semiring witness against the forward and the two-sided subgradient on the same plan, one
workload per run.

    python tools/witness_bench.py [--workload cant|scircuit|triangle] [--semiring min_plus|max_plus|max_min]
                                  [--dtype f64|f32] [--values random|quarters] [--blocks 5] [--window 0.4]
                                  [--repeats 1] [--check-rows 4000]

Workloads as in tools/subgrad_bench.py: `cant` and `scircuit` are A*A on the product's own pattern (the stand-ins of
mhspgemm.synth unless the real matrices are present); `triangle` is L*L on L's pattern, a masked plan in AUTO.

Kinds, timed in alternating blocks after warm-up (the method of tools/subgrad_bench.py: a block is enough calls for
its window to last `--window` seconds between two host clock reads after device synchronises; per kind the median of
the blocks' per-call times and the spread max - min; `--repeats R` takes the whole measurement R times in the process
-- `runs` -- and reports per kind the median of the runs' medians and their spread):
  forward      mhs_spgemm_values on the semiring plan
  subgrad_AB   mhs_spgemm_values_subgrad, both gradients: three fills and two passes of the backward's launch list
  witness      mhs_spgemm_values_witness: one fill and one pass of the same list
Values: `random` (signed, magnitudes in [0.1, 1000]: about one winner per reached entry) or `quarters` (multiples of
0.25 in [-2, 2): ties are the rule, and many winners meet in one atomic).
Before timing, the witness is checked (`witness_equal`): against a numpy reference of the rule -- per C entry the
smallest A.col among the kept products equal to it in the plan's type, -1 where there is none or the entry is the
identity -- on `--check-rows` rows spread evenly over the matrix (all rows when it has no more; 0: none), and on every
entry against the subgradient's tie count (wit >= 0 exactly where ties >= 1, and wit < A.N).  Also reported:
`tied_share`, the share of C entries with more than one winner, and `over_subgrad` / `over_forward`, the witness's
median over the other two, and `witness_le_subgrad`: whether the witness's median is at most the subgradient's in every
run.  Prints one JSON line."""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "mh-spgemm_amd", ROOT / "tools"):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import mhspgemm  # noqa: E402
from mhspgemm import _lib as L  # noqa: E402
from mhspgemm import synth  # noqa: E402
from grad_bench import lib_name  # noqa: E402
from masked_bench import lower_triangle  # noqa: E402

IDENTITY = {"min_plus": float("inf"), "max_plus": float("-inf"), "max_min": float("-inf")}


def reference_rows(sr, rows, Aptr, Acol, av, Bptr, Bcol, bv, Cptr, Ccol, cval, N):
    """The rule on the C entries of `rows` (ascending), in the dtype of the value arrays: (their positions in C, wit)."""
    ent = np.concatenate([np.arange(Aptr[r], Aptr[r + 1]) for r in rows]) if len(rows) else np.zeros(0, np.int64)
    erow = np.repeat(rows, (Aptr[rows + 1] - Aptr[rows]))
    k = Acol[ent].astype(np.int64)
    lens = (Bptr[k + 1] - Bptr[k]).astype(np.int64)
    start = np.cumsum(lens) - lens
    q = np.arange(int(lens.sum()), dtype=np.int64) - np.repeat(start, lens) + np.repeat(Bptr[k].astype(np.int64), lens)
    p = np.repeat(ent, lens)
    key = np.repeat(erow, lens).astype(np.int64) * N + Bcol[q]
    pos = np.concatenate([np.arange(Cptr[r], Cptr[r + 1]) for r in rows]) if len(rows) else np.zeros(0, np.int64)
    ckey = np.repeat(rows, (Cptr[rows + 1] - Cptr[rows])).astype(np.int64) * N + Ccol[pos]  # ascending: rows and columns ascend
    at = np.searchsorted(ckey, key)
    kept = at < len(ckey)
    kept[kept] = ckey[at[kept]] == key[kept]  # (a product outside a mask is no product)
    p, q, at = p[kept], q[kept], at[kept]
    with np.errstate(invalid="ignore"):
        prod = np.minimum(av[p], bv[q]) if sr == "max_min" else av[p] + bv[q]
    c = cval[pos][at]
    win = (prod == c) & (c != IDENTITY[sr])
    best = np.full(len(pos), np.iinfo(np.int64).max, np.int64)
    np.minimum.at(best, at[win], Acol[p[win]].astype(np.int64))
    best[best == np.iinfo(np.int64).max] = -1
    return pos, best.astype(np.int32)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workload", default="cant", choices=("cant", "scircuit", "triangle"))
    ap.add_argument("--semiring", default="min_plus", choices=tuple(IDENTITY))
    ap.add_argument("--dtype", default="f64", choices=("f32", "f64"), help="the plan's value type")
    ap.add_argument("--values", default="random", choices=("random", "quarters"))
    ap.add_argument("--n", type=int, default=50_000, help="vertices of the triangle workload's graph")
    ap.add_argument("--blocks", type=int, default=5, help="timed blocks per kind")
    ap.add_argument("--window", type=float, default=0.4, help="seconds a timed block should last")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=1, help="times the whole measurement is taken")
    ap.add_argument("--check-rows", type=int, default=4000, help="rows of the numpy reference (0: none)")
    args = ap.parse_args()
    f32, sr = args.dtype == "f32", args.semiring
    tdt = torch.float32 if f32 else torch.float64
    dev = 0
    torch.cuda.set_device(dev)
    device = f"cuda:{dev}"
    masked = args.workload == "triangle"
    if masked:
        A, source = lower_triangle(args.n), f"synth.powerlaw({args.n}), symmetrised, strictly lower; L*L on L (masked, auto)"
    else:
        A, source = synth.load_or_synth(args.workload)
    A.H2D(dev)
    tool = mhspgemm.Tool(dev)
    tool.set_stream(torch.cuda.current_stream(dev).cuda_stream)

    def sync():
        torch.cuda.synchronize(dev)

    owned = None
    if masked:
        C = mhspgemm.CSR(A.M, A.N, A.ptr, A.col, np.zeros(A.nnz))
        C.H2D(dev)
        Cptr, Ccol = A.ptr, A.col
    else:
        owned, _ = mhspgemm.spgemm(tool, A, A, timing=False)
        C = owned
        Cptr, Ccol, _ = owned.to_host()
    kw = {"masked": True, "form": "auto"} if masked else {}
    plan = mhspgemm.ValuesPlan(tool, A, A, C, dtype=tdt, semiring=sr, **kw)
    info = plan.info()
    nA, nC = A.nnz, info["nnzC"]
    out = {"workload": args.workload, "source": source, "semiring": sr, "dtype": args.dtype, "values": args.values, "M": A.M,
           "nnzA": nA, "nnzC": nC, "products": info["products"], "kept_products": info["kept_products"], "blocks": args.blocks,
           "lib": lib_name(), "classes": {k: info[k] for k in mhspgemm.core.VALUES_CLASSES}}
    rng = np.random.default_rng(17)

    def values(n):
        if args.values == "quarters":
            v = rng.integers(-8, 8, n) * 0.25
        else:
            v = rng.uniform(0.1, 1000.0, n) * rng.choice([-1.0, 1.0], n)
        return torch.from_numpy(v).to(tdt).to(device)

    av, bv = values(nA), values(nA)
    G = torch.from_numpy(rng.uniform(0.1, 1.0, nC) * rng.choice([-1.0, 1.0], nC)).to(tdt).to(device)
    nan = lambda n: torch.full((n,), float("nan"), dtype=tdt, device=device)  # noqa: E731
    cval, gA, gB = nan(nC), nan(nA), nan(nA)
    ties = torch.full((nC,), -1, dtype=torch.int32, device=device)
    wit, wit2 = (torch.full((nC,), 12345, dtype=torch.int32, device=device) for _ in range(2))
    sync()

    # ---- the check
    plan.run(av, bv, out=cval)
    plan.subgrad(G, cval, av, bv, out_A=gA, out_B=gB, ties=ties)
    plan.witness(cval, av, bv, out=wit)
    plan.witness(cval, av, bv, out=wit2)
    sync()
    checks = {"where_ties": bool(torch.equal(wit >= 0, ties >= 1)),
              "in_range": bool(torch.all((wit >= -1) & (wit < A.N)).item()),
              "two_calls_same": bool(torch.equal(wit, wit2))}
    rows = np.arange(A.M, dtype=np.int64)
    if 0 < args.check_rows < A.M:
        rows = np.unique(np.linspace(0, A.M - 1, args.check_rows).astype(np.int64))
    if args.check_rows > 0:
        hav, hbv, hc, hw = av.cpu().numpy(), bv.cpu().numpy(), cval.cpu().numpy(), wit.cpu().numpy()
        t0 = time.perf_counter()
        pos, ref = reference_rows(sr, rows, A.ptr, A.col, hav, A.ptr, A.col, hbv, np.asarray(Cptr), np.asarray(Ccol), hc, A.N)
        out["reference"] = {"rows": int(len(rows)), "entries": int(len(pos)), "seconds": round(time.perf_counter() - t0, 2),
                            "mismatches": int((hw[pos] != ref).sum())}
        checks["equals_numpy_reference"] = bool(np.array_equal(hw[pos], ref))
    out["winners"] = int(ties.sum().item())
    out["entries_with_witness"] = int((wit >= 0).sum().item())
    out["entries_with_ties"] = int((ties > 1).sum().item())
    out["tied_share"] = round(out["entries_with_ties"] / nC, 5) if nC else 0.0
    out["checks"] = checks
    out["witness_equal"] = all(checks.values())
    if not out["witness_equal"]:  # the figures first, then the failure
        print(json.dumps(out))
        raise SystemExit(f"check failed: {checks}")

    # ---- timing
    tool.set_option(L.MHS_OPT_SYNC, 0)

    def forward_calls(n):
        for _ in range(n):
            plan.run(av, bv, out=cval)

    def sub_calls(n):
        for _ in range(n):
            plan.subgrad(G, cval, av, bv, out_A=gA, out_B=gB, ties=ties)

    def wit_calls(n):
        for _ in range(n):
            plan.witness(cval, av, bv, out=wit)

    def timed(fn, n):
        sync()
        t0 = time.perf_counter()
        fn(n)
        sync()
        return (time.perf_counter() - t0) / n * 1e3  # ms per call

    kinds = [("forward", forward_calls), ("subgrad_AB", sub_calls), ("witness", wit_calls)]

    def measure():
        calls, one = {}, {}
        for name, fn in kinds:
            fn(args.warmup)
            per = timed(fn, 10)
            calls[name] = max(10, int(args.window * 1e3 / per) + 1)
            print(f"{name}: {per:.4f} ms a call, {calls[name]} calls a block", file=sys.stderr, flush=True)
        res = {name: [] for name, _ in kinds}
        for _ in range(args.blocks):
            for name, fn in kinds:
                res[name].append(timed(fn, calls[name]))
        for name, _ in kinds:
            r = res[name]
            one[name] = {"ms_median": round(statistics.median(r), 5), "ms_min": round(min(r), 5), "ms_max": round(max(r), 5),
                         "spread_ms": round(max(r) - min(r), 5), "calls_per_block": calls[name],
                         "blocks_ms": [round(x, 5) for x in r]}
        one["witness_le_subgrad"] = one["witness"]["ms_median"] <= one["subgrad_AB"]["ms_median"]
        return one

    # the whole measurement `--repeats` times: the spread between them stands beside the numbers
    out["runs"] = [measure() for _ in range(args.repeats)]
    tool.set_option(L.MHS_OPT_SYNC, 1)
    for name, _ in kinds:
        m = [run[name]["ms_median"] for run in out["runs"]]
        out[name] = {"ms_median": round(statistics.median(m), 5), "run_medians_ms": m, "run_spread_ms": round(max(m) - min(m), 5)}
    out["over_subgrad"] = round(out["witness"]["ms_median"] / out["subgrad_AB"]["ms_median"], 3)
    out["over_forward"] = round(out["witness"]["ms_median"] / out["forward"]["ms_median"], 3)
    out["witness_le_subgrad"] = all(run["witness_le_subgrad"] for run in out["runs"])
    plan.close()
    if owned is not None:
        owned.release()
    tool.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
