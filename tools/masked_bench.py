#!/usr/bin/env python3
"""masked_bench.py -- the masked product against the full call a user makes today, one workload per run.

    python tools/masked_bench.py [--workload triangle|cant|scircuit] [--blocks 5] [--window 0.4] [--full-only]
                                [--dtype f32|f64]

Workloads: `triangle` is L*L on L's pattern, L the strictly lower triangle of a symmetrised
synth.powerlaw graph with all values 1.0; `cant` and `scircuit` are A*A on A's pattern.

Kinds, timed in alternating blocks after warm-up (the method of tools/values_bench.py: a block is
enough calls for its window to last `--window` seconds between two host clock reads after device
synchronises; per kind the median of the blocks' per-call times and the spread max - min):
  full          the repeated full mhs_spgemm call (no filter counted), each C handed back to the pool
  product, dot  the masked plan in a forced form
  auto@R        the masked plan in AUTO with MHS_VAL_DOT_RATIO=R at its creation, R in 1 .. 64
Before timing, every masked plan's output is checked against the full product filtered to the mask
(the reference 1e-9 rule; mask entries outside the product exactly 0.0).

--dtype f32 makes every masked plan an FP32 plan on A's values rounded to float.  The check is then against an
FP64 masked plan (product form) on the same rounded values: every entry within 1.01 m 2^-24 S, m and S from that
plan on all-ones and on absolute values, unreached entries exactly 0.0.

--full-only times `full` alone and needs none of the masked entry points, so it runs against an
older library (MHS_LIB=/path/to/libmhspgemm.so): the parent commit's, for the comparison the table
reports.  Prints one JSON line."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "mh-spgemm_amd"):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import mhspgemm  # noqa: E402
from mhspgemm import _lib as L  # noqa: E402
from mhspgemm import synth  # noqa: E402
from mixed_rows import mixed_global_rows  # noqa: E402  (tools/mixed_rows.py: the script's own directory)

RATIOS = (1, 2, 4, 8, 16, 32, 64)


def lower_triangle(n: int, seed: int = 3) -> mhspgemm.CSR:
    G = synth.powerlaw(n, seed=seed)
    r = np.repeat(np.arange(G.M, dtype=np.int64), np.diff(G.ptr))
    c = G.col.astype(np.int64)
    off = r != c
    key = np.unique(np.maximum(r[off], c[off]) * n + np.minimum(r[off], c[off]))  # symmetrised, strictly lower
    ptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(key // n, minlength=n), out=ptr[1:])
    return mhspgemm.CSR(n, n, ptr.astype(np.int32), (key % n).astype(np.int32), np.ones(len(key)))


def filtered(Cp, Ci, Cv, Mp, Mc, N):
    rows = lambda p: np.repeat(np.arange(len(p) - 1, dtype=np.int64), np.diff(p))  # noqa: E731
    kC, kM = rows(Cp) * N + Ci, rows(Mp) * N + Mc
    pos = np.minimum(np.searchsorted(kC, kM), max(len(kC) - 1, 0))
    hit = kC[pos] == kM if len(kC) else np.zeros(len(kM), bool)
    return np.where(hit, Cv[pos], 0.0) if len(kC) else np.zeros(len(kM)), hit


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workload", default="triangle", choices=("triangle", "cant", "scircuit"))
    ap.add_argument("--n", type=int, default=50_000, help="vertices of the triangle workload's graph")
    ap.add_argument("--blocks", type=int, default=5, help="timed blocks per kind")
    ap.add_argument("--window", type=float, default=0.4, help="seconds a timed block should last")
    ap.add_argument("--warmup", type=int, default=5, help="warm-up calls per kind (1 for a kind slower than 0.1 s a call)")
    ap.add_argument("--full-only", action="store_true", help="time the repeated full call alone")
    ap.add_argument("--dtype", default="f64", choices=("f32", "f64"), help="the masked plans' value type")
    ap.add_argument("--accum", default=None, choices=("f64",), help="with --dtype f32: FP64 sums (mixed plans); the check is "
                    "then 1.01 (2^-24 |ref| + 2 m 2^-53 S) against the FP64 plan, 1.01 m 2^-24 S on global-class rows")
    args = ap.parse_args()
    f32 = args.dtype == "f32"
    mixed = args.accum == "f64"
    if mixed and not f32:
        ap.error("--accum f64 goes with --dtype f32")

    dev = 0
    torch.cuda.set_device(dev)
    if args.workload == "triangle":
        A, source = lower_triangle(args.n), f"synth.powerlaw({args.n}), symmetrised, strictly lower, values 1.0"
    else:
        A, source = synth.load_or_synth(args.workload)
    flop = mhspgemm.flop_count_np(A.col, A.ptr)
    A.H2D(dev)
    tool = mhspgemm.Tool(dev)
    tool.set_stream(torch.cuda.current_stream(dev).cuda_stream)

    def sync():
        torch.cuda.synchronize(dev)

    out = {"workload": args.workload, "source": source, "M": A.M, "nnzA": A.nnz, "products": int(flop),
           "blocks": args.blocks, "lib": L.lib_path(), "dtype": args.dtype, "accum": args.accum}
    C, _ = mhspgemm.spgemm(tool, A, A, timing=False)
    out["nnzC"] = C.nnz
    print(f"{args.workload}: nnz(A) {A.nnz}, {flop} products, nnz(C) {C.nnz}", file=sys.stderr, flush=True)

    plans = {}
    a32 = res32 = None
    if not args.full_only and f32:  # the FP32 plans' operands, and their reference: an FP64 plan on the rounded values
        a32 = torch.from_numpy(A.val.astype(np.float32)).to(f"cuda:{dev}")
        res32 = torch.empty(A.nnz, dtype=torch.float32, device=f"cuda:{dev}")
        mask64 = mhspgemm.CSR(A.M, A.N, A.ptr, A.col, np.zeros(A.nnz))
        mask64.H2D(dev)
        plan64 = mhspgemm.ValuesPlan(tool, A, A, mask64, masked=True, form="product")
        ref, cnt, sab = (torch.empty(A.nnz, dtype=torch.float64, device=f"cuda:{dev}") for _ in range(3))
        ones = torch.ones(A.nnz, dtype=torch.float64, device=f"cuda:{dev}")
        sync()
        plan64.run(a32.double(), a32.double(), out=ref)
        plan64.run(ones, ones, out=cnt)
        plan64.run(a32.double().abs(), a32.double().abs(), out=sab)
        sync()
        plan64.close()
    if not args.full_only:
        Cp, Ci, Cv = C.to_host()
        want, hit = filtered(Cp, Ci, Cv, A.ptr, A.col, A.N)
        out["mask_entries"] = A.nnz
        out["mask_entries_reached"] = int(hit.sum())
        mask = mhspgemm.CSR(A.M, A.N, A.ptr, A.col, np.zeros(A.nnz))
        mask.H2D(dev)
        kinds = [("product", "product", None), ("dot", "dot", None)] + [(f"auto@{r}", "auto", r) for r in RATIOS]
        out["plans"] = {}
        for name, form, ratio in kinds:
            if ratio is None:
                os.environ.pop("MHS_VAL_DOT_RATIO", None)
            else:
                os.environ["MHS_VAL_DOT_RATIO"] = str(ratio)  # read by the library at plan creation
            plan = mhspgemm.ValuesPlan(tool, A, A, mask, masked=True, form=form, dtype="float32" if f32 else "float64",
                                       **({"accum": "float64"} if mixed else {}))
            info = plan.info()
            if f32:
                res32.fill_(float("nan"))
                sync()
                plan.run(a32, a32, out=res32)
                sync()
                assert not torch.isnan(res32).any().item(), f"{name}: an entry was not written"
                bound = 1.01 * cnt * 2.0 ** -24 * sab
                if mixed:  # (a dot row that the product-form rule would send to the global class keeps the looser bound)
                    rows = mixed_global_rows(A.ptr, A.col, 1)
                    assert int(rows.sum()) >= info["global"]
                    glob = torch.from_numpy(np.repeat(rows, np.diff(A.ptr))).to(f"cuda:{dev}")
                    bound = torch.where(glob, bound, 1.01 * (2.0 ** -24 * ref.abs() + 2 * cnt * 2.0 ** -53 * sab))
                assert torch.all((res32.double() - ref).abs() <= bound).item(), f"{name}: outside its bound"
                assert torch.all(res32[cnt == 0] == 0).item(), f"{name}: an unreached mask entry is not 0.0"
            else:
                res = torch.full((A.nnz,), float("nan"), dtype=torch.float64, device=f"cuda:{dev}")
                plan.run(out=res)
                sync()
                got = res.cpu().numpy()
                assert mhspgemm.compare_ref(A.ptr, A.col, want, A.ptr, A.col, got), f"{name}: outside the 1e-9 rule"
                assert np.all(got[~hit] == 0.0), f"{name}: an unreached mask entry is not 0.0"
            plans[name] = plan
            print(f"{name}: checked, dot rows {info['dot']}", file=sys.stderr, flush=True)
            out["plans"][name] = {"dot_rows": info["dot"], "kept_products": info["kept_products"],
                                  "plan_bytes": info["plan_bytes"],
                                  "classes": {k: info[k] for k in mhspgemm.core.VALUES_CLASSES}}
        os.environ.pop("MHS_VAL_DOT_RATIO", None)
        out["checked"] = "every plan against the full product filtered to the mask: the reference 1e-9 rule, misses exactly 0.0"
        if f32:
            out["checked"] = ("every plan against an FP64 masked plan on the same rounded values: every entry within "
                              "1.01 m 2^-24 S, misses exactly 0.0")
        if mixed:
            out["checked"] = ("every plan against an FP64 masked plan on the same rounded values: every entry within "
                              "1.01 (2^-24 |ref| + 2 m 2^-53 S), global-class rows within 1.01 m 2^-24 S, misses exactly 0.0")

    # ---- timing
    tool.set_option(L.MHS_OPT_SYNC, 0)
    state = {"C": None}

    def full_calls(n):
        for _ in range(n):
            if state["C"] is not None:
                state["C"].release()
            state["C"], _ = mhspgemm.spgemm(tool, A, A, timing=False)

    def masked_calls(plan):
        def fn(n):
            for _ in range(n):
                plan.run(a32, a32, out=res32)  # (FP64: all None, the operands' and the mask's own values)
        return fn

    def timed(fn, n):
        sync()
        t0 = time.perf_counter()
        fn(n)
        sync()
        return (time.perf_counter() - t0) / n * 1e3  # ms per call

    kinds = [("full", full_calls)] + [(name, masked_calls(plan)) for name, plan in plans.items()]
    calls = {}
    for name, fn in kinds:
        # (a forced dot plan can take seconds a call on hub rows: warm up and size the block by its first call)
        first = timed(fn, 1)
        few = first > 100.0
        fn(1 if few else args.warmup)
        per = timed(fn, 2 if few else 20)
        calls[name] = max(1 if few else 20, int(args.window * 1e3 / per) + 1)
        print(f"{name}: {per:.4f} ms a call, {calls[name]} calls a block", file=sys.stderr, flush=True)
    res = {name: [] for name, _ in kinds}
    for _ in range(args.blocks):
        for name, fn in kinds:
            res[name].append(timed(fn, calls[name]))
    tool.set_option(L.MHS_OPT_SYNC, 1)
    for name, _ in kinds:
        r = res[name]
        out[name] = {"ms_median": round(statistics.median(r), 5), "ms_min": round(min(r), 5), "ms_max": round(max(r), 5),
                     "spread_ms": round(max(r) - min(r), 5), "calls_per_block": calls[name],
                     "blocks_ms": [round(x, 5) for x in r]}
    if state["C"] is not None:
        state["C"].release()
    for plan in plans.values():
        plan.close()
    C.release()
    tool.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
