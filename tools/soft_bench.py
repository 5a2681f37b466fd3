#!/usr/bin/env python3
"""soft_bench.py -- the soft semiring plans (smooth="lse") against the hard plan of the same semiring, and their gradient
against the subgradient and the plus-times backward of the same pattern and type, one workload per run.

    python tools/soft_bench.py [--workload cant|scircuit|triangle] [--semiring min_plus|max_plus] [--dtype f64|f32]
                               [--blocks 5] [--window 0.4]

Workloads as in tools/subgrad_bench.py: `cant` and `scircuit` are A*A on the product's own pattern (the stand-ins of
mhspgemm.synth unless the real matrices are present); `triangle` is L*L on L's pattern, a masked plan in AUTO.

Kinds, timed in alternating blocks after warm-up (the method of tools/values_bench.py: a block is enough calls for its
window to last `--window` seconds between two host clock reads after device synchronises; per kind the median of the
blocks' per-call times and the spread max - min):
  soft_forward   mhs_spgemm_values on the smoothed plan (two walks: max, then sum of exp)
  hard_forward   ... on the hard plan of the same semiring
  softgrad_A / softgrad_B / softgrad_AB   mhs_spgemm_values_softgrad: dAval only, dBval only, both (one pass)
  subgrad_A / _B / _AB                    mhs_spgemm_values_subgrad on the hard plan (two passes)
  pt_grad_A / _B / _AB                    mhs_spgemm_values_grad on a plus-times plan of the same patterns and type
Values are uniform in [-8, 8].  Before timing, the calls are checked on the device (`check_pass`): every entry written;
the soft result equal to the hard one where that is the identity and otherwise between it and log(most) on the soft side
of it, `most` the most products of an entry (the longest A row bounds it); the gradient mass -- sum(dA) and sum(dB)
against the sum of G over the finite entries, the weights of an entry being softmax weights -- to
(most + 40) u of the sum of |G|; the one-sided calls' dA the bits of the two-sided call's.
Also reported: `soft_over_hard`, and each soft gradient time over the subgradient's and over the plus-times backward's.
Prints one JSON line."""
from __future__ import annotations

import argparse
import json
import math
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

IDENTITY = {"min_plus": float("inf"), "max_plus": float("-inf")}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workload", default="cant", choices=("cant", "scircuit", "triangle"))
    ap.add_argument("--semiring", default="min_plus", choices=tuple(IDENTITY))
    ap.add_argument("--dtype", default="f64", choices=("f32", "f64"), help="the plan's value type")
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
    soft = mhspgemm.ValuesPlan(tool, A, A, C, dtype=tdt, semiring=sr, smooth="lse", **kw)
    hard = mhspgemm.ValuesPlan(tool, A, A, C, dtype=tdt, semiring=sr, **kw)
    plain = mhspgemm.ValuesPlan(tool, A, A, C, dtype=tdt, **kw)
    info, hinfo = soft.info(), hard.info()
    nA, nC = A.nnz, info["nnzC"]
    out = {"workload": args.workload, "source": source, "semiring": sr, "smooth": info["smooth"], "dtype": args.dtype, "M": A.M,
           "nnzA": nA, "nnzC": nC, "products": info["products"], "kept_products": info["kept_products"], "blocks": args.blocks,
           "lib": lib_name(), "classes": {k: info[k] for k in mhspgemm.core.VALUES_CLASSES},
           "hard_classes": {k: hinfo[k] for k in mhspgemm.core.VALUES_CLASSES}}
    rng = np.random.default_rng(17)
    av, bv = (torch.from_numpy(rng.uniform(-8.0, 8.0, nA)).to(tdt).to(device) for _ in range(2))
    G = torch.from_numpy(rng.uniform(0.1, 1.0, nC) * rng.choice([-1.0, 1.0], nC)).to(tdt).to(device)
    nan = lambda n: torch.full((n,), float("nan"), dtype=tdt, device=device)  # noqa: E731
    cval, hval, gA, gB, oA, oB = nan(nC), nan(nC), nan(nA), nan(nA), nan(nA), nan(nA)
    ties = torch.full((nC,), -1, dtype=torch.int32, device=device)
    sync()

    # ---- the check
    soft.run(av, bv, out=cval)
    hard.run(av, bv, out=hval)
    soft.softgrad(G, cval, av, bv, out_A=gA, out_B=gB)
    sync()
    u = 2.0 ** -24 if f32 else 2.0 ** -53
    most = int(np.diff(A.ptr).max())  # an entry's products: at most one per A entry of its row (A has no duplicates)
    live = torch.isfinite(hval)
    sg = -1.0 if sr == "min_plus" else 1.0
    gap = (sg * (cval.double() - hval.double()))[live]  # 0 <= gap <= log(products of the entry)
    slack = 40 * u * (1 + hval.double().abs()[live])
    mass = float(G[live].double().sum())
    room = (most + 40) * u * float(G[live].double().abs().sum())
    sA, sB = float(gA.double().sum()), float(gB.double().sum())
    checks = {"written": not (torch.isnan(cval).any() or torch.isnan(gA).any() or torch.isnan(gB).any()).item(),
              "identity_where_hard": bool(torch.equal(cval[~live], hval[~live])),
              "between_hard_and_log": bool(torch.all(gap >= -slack).item() and torch.all(gap <= math.log(max(most, 1)) + slack).item()),
              "mass": bool(max(abs(sA - mass), abs(sB - mass)) <= room)}
    for need_a, need_b in ((True, False), (False, True)):
        oA.fill_(float("nan"))
        oB.fill_(float("nan"))
        sync()
        soft.softgrad(G, cval, av, bv, need_A=need_a, need_B=need_b, out_A=oA, out_B=oB)
        sync()
        if need_a:
            checks["dA_alone_same_bits"] = bool(torch.equal(oA, gA) and torch.isnan(oB).all().item())
        else:
            checks["dB_alone"] = bool(torch.isnan(oA).all().item() and abs(float(oB.double().sum()) - sB) <= 2 * room)
    out["max_gap"] = float(gap.max().item()) if gap.numel() else 0.0
    out["mass_gap_over_room"] = round(max(abs(sA - mass), abs(sB - mass)) / room, 4) if room > 0 else 0.0
    out["checks"] = checks
    out["check_pass"] = all(checks.values())
    if not out["check_pass"]:  # the figures first, then the failure
        print(json.dumps(out))
        raise SystemExit(f"check failed: {checks}")

    # ---- timing
    tool.set_option(L.MHS_OPT_SYNC, 0)

    def forward_calls(plan, dst):
        def fn(n):
            for _ in range(n):
                plan.run(av, bv, out=dst)
        return fn

    def soft_calls(need_a, need_b):
        def fn(n):
            for _ in range(n):
                soft.softgrad(G, cval, av, bv, need_A=need_a, need_B=need_b, out_A=gA, out_B=gB)
        return fn

    def sub_calls(need_a, need_b):
        def fn(n):
            for _ in range(n):
                hard.subgrad(G, hval, av, bv, need_A=need_a, need_B=need_b, out_A=oA, out_B=oB, ties=ties)
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
    kinds = [("soft_forward", forward_calls(soft, cval)), ("hard_forward", forward_calls(hard, hval))]
    for s, na, nb in sides:
        kinds += [(f"softgrad_{s}", soft_calls(na, nb)), (f"subgrad_{s}", sub_calls(na, nb)), (f"pt_grad_{s}", pt_calls(na, nb))]
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
    out["soft_over_hard"] = round(out["soft_forward"]["ms_median"] / out["hard_forward"]["ms_median"], 3)
    out["over_subgrad"] = {s: round(out[f"softgrad_{s}"]["ms_median"] / out[f"subgrad_{s}"]["ms_median"], 3) for s, _, _ in sides}
    out["over_pt"] = {s: round(out[f"softgrad_{s}"]["ms_median"] / out[f"pt_grad_{s}"]["ms_median"], 3) for s, _, _ in sides}
    for plan in (soft, hard, plain):
        plan.close()
    if owned is not None:
        owned.release()
    tool.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
