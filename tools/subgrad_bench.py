#!/usr/bin/env python3
"""subgrad_bench.py -- the semiring subgradient against the forward on the same plan and against the plus-times
backward of the same pattern and type, one workload per run.

    python tools/subgrad_bench.py [--workload cant|scircuit|triangle] [--semiring min_plus|max_plus|max_min]
                                  [--dtype f64|f32] [--values random|quarters] [--blocks 5] [--window 0.4]

Workloads as in tools/grad_bench.py: `cant` and `scircuit` are A*A on the product's own pattern (the stand-ins of
mhspgemm.synth unless the real matrices are present); `triangle` is L*L on L's pattern, a masked plan in AUTO.

Kinds, timed in alternating blocks after warm-up (the method of tools/values_bench.py: a block is enough calls for its
window to last `--window` seconds between two host clock reads after device synchronises; per kind the median of the
blocks' per-call times and the spread max - min):
  forward      mhs_spgemm_values on the semiring plan
  subgrad_A    mhs_spgemm_values_subgrad, dAval only (pass 1's integer atomics, no float atomics)
  subgrad_B    ... dBval only (one float atomic per winner)
  subgrad_AB   ... both
  pt_grad_A / pt_grad_B / pt_grad_AB   mhs_spgemm_values_grad on a plus-times plan of the same patterns and type, for scale
Values: `random` (signed, magnitudes in [0.1, 1000]: about one winner per reached entry) or `quarters` (multiples of
0.25 in [-2, 2): ties are the rule).  Before timing, the call is checked on the device (`check_pass`): ties >= 1 on
every entry whose forward value is neither NaN nor the identity and 0 elsewhere; the gradient mass -- under the _plus
semirings sum(dA) and sum(dB), under max_min their sum, against the sum of G over the entries with winners, to
(most + 1) u of the sum of |G| there, `most` the longest B row or fullest A column (every entry is within
(m + 1) u S of its exact sum); the one-sided calls' dA the bits of the two-sided call's, their ties equal.
Also reported: winners (sum of ties), and `over_pt`: each subgradient time over the plus-times backward's.
Prints one JSON line."""
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
    else:
        owned, _ = mhspgemm.spgemm(tool, A, A, timing=False)
        C = owned
    kw = {"masked": True, "form": "auto"} if masked else {}
    plan = mhspgemm.ValuesPlan(tool, A, A, C, dtype=tdt, semiring=sr, **kw)
    plain = mhspgemm.ValuesPlan(tool, A, A, C, dtype=tdt, **kw)
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
    cval, gA, gB, oA, oB = nan(nC), nan(nA), nan(nA), nan(nA), nan(nA)
    ties, ties1 = (torch.full((nC,), -1, dtype=torch.int32, device=device) for _ in range(2))
    sync()

    # ---- the check
    plan.run(av, bv, out=cval)
    plan.subgrad(G, cval, av, bv, out_A=gA, out_B=gB, ties=ties)
    sync()
    live = ~torch.isnan(cval) & (cval != IDENTITY[sr])
    won = ties > 0
    most = max(int(np.diff(A.ptr).max()), int(np.bincount(A.col).max()))
    u = 2.0 ** -24 if f32 else 2.0 ** -53
    mass = float(G[won].double().sum())
    room = (most + 1) * u * float(G[won].double().abs().sum())
    sA, sB = float(gA.double().sum()), float(gB.double().sum())
    gaps = [abs(sA + sB - mass) / 2] if sr == "max_min" else [abs(sA - mass), abs(sB - mass)]
    checks = {"written": not (torch.isnan(gA).any() or torch.isnan(gB).any()).item(),
              "ties_where_live": bool(torch.all(ties[live] >= 1).item() and torch.all(ties[~live] == 0).item()),
              "mass": bool(max(gaps) <= room)}
    for need_a, need_b in ((True, False), (False, True)):
        oA.fill_(float("nan"))
        oB.fill_(float("nan"))
        sync()
        plan.subgrad(G, cval, av, bv, need_A=need_a, need_B=need_b, out_A=oA, out_B=oB, ties=ties1)
        sync()
        if need_a:
            checks["dA_alone_same_bits"] = bool(torch.equal(oA, gA) and torch.isnan(oB).all().item())
        else:
            checks["dB_alone"] = bool(torch.isnan(oA).all().item() and abs(float(oB.double().sum()) - sB) <= 2 * room)
        checks["ties_same"] = checks.get("ties_same", True) and bool(torch.equal(ties1, ties))
    out["winners"] = int(ties.sum().item())
    out["entries_with_ties"] = int((ties > 1).sum().item())
    out["mass_gap_over_room"] = round(max(gaps) / room, 4) if room > 0 else 0.0
    out["checks"] = checks
    out["check_pass"] = all(checks.values())
    if not out["check_pass"]:  # the figures first, then the failure
        print(json.dumps(out))
        raise SystemExit(f"check failed: {checks}")

    # ---- timing
    tool.set_option(L.MHS_OPT_SYNC, 0)

    def forward_calls(n):
        for _ in range(n):
            plan.run(av, bv, out=cval)

    def sub_calls(need_a, need_b):
        def fn(n):
            for _ in range(n):
                plan.subgrad(G, cval, av, bv, need_A=need_a, need_B=need_b, out_A=gA, out_B=gB, ties=ties)
        return fn

    def pt_calls(need_a, need_b):
        def fn(n):
            for _ in range(n):
                plain.grad(G, av, bv, need_A=need_a, need_B=need_b, out_A=oA, out_B=oB)
        return fn

    def timed(fn, n):
        sync()
        t0 = time.perf_counter()
        fn(n)
        sync()
        return (time.perf_counter() - t0) / n * 1e3  # ms per call

    sides = (("A", True, False), ("B", False, True), ("AB", True, True))
    kinds = [("forward", forward_calls)]
    for s, na, nb in sides:
        kinds += [(f"subgrad_{s}", sub_calls(na, nb)), (f"pt_grad_{s}", pt_calls(na, nb))]
    calls = {}
    for name, fn in kinds:
        fn(args.warmup)
        per = timed(fn, 10)
        calls[name] = max(10, int(args.window * 1e3 / per) + 1)
        print(f"{name}: {per:.4f} ms a call, {calls[name]} calls a block", file=sys.stderr, flush=True)
    res = {name: [] for name, _ in kinds}
    for _ in range(args.blocks):
        for name, fn in kinds:
            res[name].append(timed(fn, calls[name]))
    tool.set_option(L.MHS_OPT_SYNC, 1)
    for name, _ in kinds:
        r = res[name]
        out[name] = {"ms_median": round(statistics.median(r), 5), "ms_min": round(min(r), 5), "ms_max": round(max(r), 5),
                     "spread_ms": round(max(r) - min(r), 5), "calls_per_block": calls[name], "blocks_ms": [round(x, 5) for x in r]}
    out["over_pt"] = {s: round(out[f"subgrad_{s}"]["ms_median"] / out[f"pt_grad_{s}"]["ms_median"], 3) for s, _, _ in sides}
    out["over_forward"] = {s: round(out[f"subgrad_{s}"]["ms_median"] / out["forward"]["ms_median"], 3) for s, _, _ in sides}
    plan.close()
    plain.close()
    if owned is not None:
        owned.release()
    tool.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
