#!/usr/bin/env python3
"""grad_bench.py -- the values backward against the values call on the same plan, one workload per run.

    python tools/grad_bench.py [--workload cant|scircuit|triangle] [--blocks 5] [--window 0.4] [--dtype f32|f64]
                               [--accum f64] [--batch NB --width W]

Workloads: `cant` and `scircuit` are A*A on the product's own pattern (the stand-ins of
mhspgemm.synth unless the real matrices are present); `triangle` is L*L on L's pattern, a masked plan
in AUTO, L the strictly lower triangle of a symmetrised synth.powerlaw graph (tools/masked_bench.py's).

Kinds, timed in alternating blocks after warm-up (the method of tools/values_bench.py: a block is
enough calls for its window to last `--window` seconds between two host clock reads after device
synchronises; per kind the median of the blocks' per-call times and the spread max - min):
  forward   mhs_spgemm_values
  grad_A    mhs_spgemm_values_grad, dAval only (no atomics)
  grad_B    ... dBval only (one FP64 atomic per kept product)
  grad_AB   ... both
Before timing, every output is checked against the forward through the adjoint identity: with X, Y
fresh positive values, <G, run(X, Bval)> = <grad_A, X> and <G, run(Aval, Y)> = <grad_B, Y> to 1e-9
relative (the same terms summed in another order), for the one-sided calls and for the call with both.
--dtype f32: an FP32 plan on float32 values.  The identities then hold to 2.02 m 2^-24 relative, m the most
products any output entry sums (the values are positive, so each side is within m 2^-24 of the exact sum; m
from an FP64 plan on all-ones values, B's longest row and A's fullest column); that plan's rows by class are
reported as `classes_f64`, and the dB side's atomic bytes are 4 a product.
--accum f64 with --dtype f32: a mixed plan -- FP64 sums in the forward, whose rows by class are then
the FP64 plan's; the backward is the FP32 plan's kernels on that launch list, and the FP32 tolerances stand.
Also reported: the dB side's atomic bytes per second, 8 * kept_products / the grad_B time, and
`masked_alternative_products`: what the two gradients would walk as masked products of their own,
dA = (G*B^T)<A>: the sum over C's entries (i, j) of len(B^T row j), and dB = (A^T*G)<B>: the sum over
A's entries (i, k) of len(C row i) = sum_i nnzA(i) * nnzC(i)  ("not done").
Prints one JSON line.

--batch NB [--width W] (default: no batch, the line above): the batched backward instead, one configuration per run.
  (a) the loop: NB calls of mhs_spgemm_values_grad on a width-1 plan, one per value and cotangent set -- what a
      caller does without the batched entry point;
  (b) one mhs_spgemm_values_grad_batched call on all NB sets through a plan of width W: ceil(NB / W) passes.
Each of dA only, dB only and both is timed as a pair of kinds, (a) and (b) in alternating blocks as above (a call of
(a) is the whole loop); (b) counts as faster or slower only beyond the larger spread of the pair.  Before timing every
set of (b), both gradients, is checked: FP64 against (a)'s result for the set -- both lie within 1.01 m 2^-53 S of
the exact sum, so within twice that of each other; FP32 against an FP64 width-1 plan on the same rounded values,
within 1.01 m 2^-24 S.  m comes from an FP64 backward on all-ones; the values are positive, so S is the FP64 result
itself.  The rows by class at width W and at width 1 stand beside the times."""
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
from masked_bench import lower_triangle  # noqa: E402


def lib_name() -> str:
    """The library's path, relative to the repository when it is the one built in it."""
    path = Path(L.lib_path()).resolve()
    return str(path.relative_to(ROOT)) if ROOT in path.parents else str(path)


def batched(args):
    """--batch NB --width W: the loop of NB unbatched backward calls against the one batched call."""
    f32, W, NB = args.dtype == "f32", args.width, args.batch
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
        C = A
    else:
        owned, _ = mhspgemm.spgemm(tool, A, A, timing=False)
        C = owned
    kw = {"masked": True, "form": "auto"} if masked else {}
    if args.accum == "f64":  # mixed plans: the backward is the FP32 plans' on the launch list planned at 8 W bytes
        kw["accum"] = "float64"
    wide = mhspgemm.ValuesPlan(tool, A, A, C, dtype=tdt, width=W, **kw)
    one = mhspgemm.ValuesPlan(tool, A, A, C, dtype=tdt, width=1, **kw)
    iw, i1 = wide.info(), one.info()
    nC, nnz = iw["nnzC"], A.nnz
    out = {"workload": args.workload, "source": source, "M": A.M, "nnzA": nnz, "nnzC": nC, "products": iw["products"],
           "kept_products": iw["kept_products"], "dtype": args.dtype, "accum": args.accum, "width": W, "batch": NB,
           "blocks": args.blocks, "lib": lib_name(), "classes": {k: iw[k] for k in mhspgemm.core.VALUES_CLASSES},
           "classes_width1": {k: i1[k] for k in mhspgemm.core.VALUES_CLASSES}}
    rng = np.random.default_rng(17)
    av, bv, G = (torch.from_numpy(rng.uniform(0.1, 1.0, (NB, n))).to(tdt).to(device) for n in (nnz, nnz, nC))
    nan = lambda n: torch.full((NB, n), float("nan"), dtype=tdt, device=device)  # noqa: E731
    resA, resB, loopA, loopB = nan(nnz), nan(nnz), nan(nnz), nan(nnz)
    sync()

    def batched_call(need_a, need_b):
        return lambda: wide.grad_batched(G, av, bv, need_A=need_a, need_B=need_b, out_A=resA, out_B=resB)

    def loop_call(need_a, need_b):
        def fn():
            for b in range(NB):
                one.grad(G[b], av[b], bv[b], need_A=need_a, need_B=need_b, out_A=loopA[b], out_B=loopB[b])
        return fn

    # ---- the check of every set, both gradients
    batched_call(True, True)()
    loop_call(True, True)()
    ref64 = mhspgemm.ValuesPlan(tool, A, A, C, **kw)
    ones_a, ones_c = torch.ones(nnz, dtype=torch.float64, device=device), torch.ones(nC, dtype=torch.float64, device=device)
    sync()
    cntA, cntB = ref64.grad(ones_c, ones_a, ones_a)
    sync()
    for t in (resA, resB, loopA, loopB):
        assert not torch.isnan(t).any().item(), "an entry of a requested output was not written"
    worst = []  # per set: the largest error over its bound, over both gradients
    for b in range(NB):
        a64, b64, g64 = av[b].double(), bv[b].double(), G[b].double()
        sync()  # (torch's conversions run on its stream, the library's calls on the tool's: each waits for the other)
        refA, refB = ref64.grad(g64, a64, b64)  # (positive values: S is the reference itself)
        sync()
        w = 0.0
        for got, loop, ref, cnt in ((resA[b], loopA[b], refA, cntA), (resB[b], loopB[b], refB, cntB)):
            if f32:
                err, bound = (got.double() - ref).abs(), 1.01 * cnt * 2.0 ** -24 * ref
            else:
                err, bound = (got - loop).abs(), 2 * 1.01 * cnt * 2.0 ** -53 * ref
            assert torch.all(got[cnt == 0] == 0).item(), f"set {b}: an unreached entry is not 0"
            if bool((cnt > 0).any()):
                w = max(w, float((err[cnt > 0] / bound[cnt > 0]).max().item()))
        worst.append(round(w, 4))
    ref64.close()
    out["checked"] = (f"every one of {NB} sets, dA and dB: " +
                      ("against an FP64 width-1 plan on the same rounded values, within 1.01 m 2^-24 S" if f32
                       else "against the unbatched call, within 2 x 1.01 m 2^-53 S"))
    out["check_worst_err_over_bound"] = worst
    out["check_pass"] = bool(max(worst) <= 1.0)
    if not out["check_pass"]:  # the figures first, then the failure
        print(json.dumps(out))
        raise SystemExit(f"check failed: worst error / bound per set {worst}")

    # ---- timing: per side, the loop and the batched call in alternating blocks
    tool.set_option(L.MHS_OPT_SYNC, 0)

    def timed(fn, n):
        sync()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        sync()
        return (time.perf_counter() - t0) / n * 1e3  # ms per call

    for side, need_a, need_b in (("grad_A", True, False), ("grad_B", False, True), ("grad_AB", True, True)):
        kinds = [("loop", loop_call(need_a, need_b)), ("batched", batched_call(need_a, need_b))]
        calls, blocks = {}, {name: [] for name, _ in kinds}
        for name, fn in kinds:
            timed(fn, args.warmup)
            calls[name] = max(10, int(args.window * 1e3 / timed(fn, 10)) + 1)
        for _ in range(args.blocks):
            for name, fn in kinds:
                blocks[name].append(timed(fn, calls[name]))
        r = {}
        for name, _ in kinds:
            x = blocks[name]
            r[name] = {"ms_median": round(statistics.median(x), 5), "ms_min": round(min(x), 5), "ms_max": round(max(x), 5),
                       "spread_ms": round(max(x) - min(x), 5), "calls_per_block": calls[name], "blocks_ms": [round(v, 5) for v in x]}
        spread = max(r["loop"]["spread_ms"], r["batched"]["spread_ms"])
        gain = r["loop"]["ms_median"] - r["batched"]["ms_median"]
        r["batched_vs_loop"] = {"gain_ms": round(gain, 5), "spread_ms": spread,
                                "ratio": round(r["batched"]["ms_median"] / r["loop"]["ms_median"], 4),
                                "faster_beyond_spread": bool(gain > spread), "slower_beyond_spread": bool(-gain > spread)}
        out[side] = r
        print(f"{side}: loop {r['loop']['ms_median']:.4f} ms, batched {r['batched']['ms_median']:.4f} ms", file=sys.stderr, flush=True)
    tool.set_option(L.MHS_OPT_SYNC, 1)
    wide.close()
    one.close()
    if owned is not None:
        owned.release()
    tool.close()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workload", default="cant", choices=("cant", "scircuit", "triangle"))
    ap.add_argument("--n", type=int, default=50_000, help="vertices of the triangle workload's graph")
    ap.add_argument("--blocks", type=int, default=5, help="timed blocks per kind")
    ap.add_argument("--window", type=float, default=0.4, help="seconds a timed block should last")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--dtype", default="f64", choices=("f32", "f64"), help="the plan's value type")
    ap.add_argument("--accum", default=None, choices=("f64",), help="with --dtype f32: FP64 sums in the forward (a mixed plan); "
                    "its backward is the FP32 plan's, and the FP32 tolerances stand")
    ap.add_argument("--batch", type=int, default=0, help="value sets (NB) of the batched backward; 0: the unbatched line")
    ap.add_argument("--width", type=int, default=None, choices=(1, 2, 4), help="the batched plan's width (with --batch; default 4)")
    args = ap.parse_args()
    if args.batch < 0 or (args.width is not None and args.batch == 0):
        ap.error("--batch: at least one value set; --width goes with --batch")
    if args.accum == "f64" and args.dtype != "f32":
        ap.error("--accum f64 goes with --dtype f32")
    if args.batch:
        args.width = args.width or 4
        return batched(args)
    f32 = args.dtype == "f32"
    tdtype = torch.float32 if f32 else torch.float64

    dev = 0
    torch.cuda.set_device(dev)
    device = f"cuda:{dev}"
    masked = args.workload == "triangle"
    if masked:
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
           "blocks": args.blocks, "lib": lib_name(), "dtype": args.dtype, "accum": args.accum}
    kw = {"dtype": "float32"} if f32 else {}  # (an older library's wrapper has no dtype argument)
    if args.accum == "f64":
        kw["accum"] = "float64"
    if masked:
        C = mhspgemm.CSR(A.M, A.N, A.ptr, A.col, np.zeros(A.nnz))
        C.H2D(dev)
        plan = mhspgemm.ValuesPlan(tool, A, A, C, masked=True, form="auto", **kw)
    else:
        C, _ = mhspgemm.spgemm(tool, A, A, timing=False)
        plan = mhspgemm.ValuesPlan(tool, A, A, C, **kw)
    info = plan.info()
    tol = 1e-9
    if f32:
        plan64 = mhspgemm.ValuesPlan(tool, A, A, C, masked=True, form="auto") if masked else mhspgemm.ValuesPlan(tool, A, A, C)
        i64 = plan64.info()
        out["classes_f64"] = {k: i64[k] for k in mhspgemm.core.VALUES_CLASSES}
        ones = torch.ones(A.nnz, dtype=torch.float64, device=device)
        cnt = torch.empty(info["nnzC"], dtype=torch.float64, device=device)
        torch.cuda.synchronize(dev)
        plan64.run(ones, ones, out=cnt)
        torch.cuda.synchronize(dev)
        most = max(int(cnt.max().item()) if info["nnzC"] else 0, int(np.diff(A.ptr).max()), int(np.bincount(A.col).max()))
        plan64.close()
        tol = 2.02 * most * 2.0 ** -24
        out["most_products_per_entry"] = most
    out.update({"nnzC": info["nnzC"], "kept_products": info["kept_products"], "plan_bytes": info["plan_bytes"],
                "classes": {k: info[k] for k in mhspgemm.core.VALUES_CLASSES}})
    Cp, Ci = (A.ptr, A.col) if masked else C.to_host()[:2]
    out["masked_alternative_products"] = {
        "dA": int(np.bincount(A.col, minlength=A.N).astype(np.int64)[Ci].sum()),
        "dB": int((np.diff(A.ptr).astype(np.int64) * np.diff(Cp).astype(np.int64)).sum())}
    del Cp, Ci
    print(f"{args.workload}: nnz(A) {A.nnz}, {flop} products, {info['kept_products']} kept, nnz(C) {info['nnzC']}",
          file=sys.stderr, flush=True)

    gen = torch.Generator(device=device).manual_seed(17)
    rnd = lambda n: (torch.rand(n, dtype=torch.float64, device=device, generator=gen) * 0.9 + 0.1).to(tdtype)  # noqa: E731
    av, bv, X, Y, G = rnd(A.nnz), rnd(A.nnz), rnd(A.nnz), rnd(A.nnz), rnd(info["nnzC"])
    res_c = torch.empty(info["nnzC"], dtype=tdtype, device=device)
    gA, gB = (torch.full((A.nnz,), float("nan"), dtype=tdtype, device=device) for _ in range(2))
    dot = lambda x, y: float((x.double() * y.double()).sum())  # noqa: E731
    sync()  # (torch's default stream has the handle 0: the tool runs on its own stream, ordered by device synchronises)

    # ---- the check: the adjoint identity against the forward, for every kind of call
    plan.run(X, bv, out=res_c)
    lhs_a = dot(G, res_c)
    plan.run(av, Y, out=res_c)
    lhs_b = dot(G, res_c)
    worst = 0.0
    for need_a, need_b in ((True, False), (False, True), (True, True)):
        gA.fill_(float("nan"))
        gB.fill_(float("nan"))
        sync()
        plan.grad(G, av, bv, need_A=need_a, need_B=need_b, out_A=gA, out_B=gB)
        sync()
        for need, g, other, lhs in ((need_a, gA, X, lhs_a), (need_b, gB, Y, lhs_b)):
            if not need:
                continue
            assert not torch.isnan(g).any().item(), "an entry of a requested output was not written"
            rel = abs(dot(g, other) - lhs) / lhs
            assert rel <= tol, f"adjoint identity off by {rel:.3e} (need_A={need_a}, need_B={need_b})"
            worst = max(worst, rel)
    out["checked"] = f"adjoint identity against the forward, one-sided and two-sided calls: worst relative gap {worst:.2e}"

    # ---- timing
    tool.set_option(L.MHS_OPT_SYNC, 0)

    def forward_calls(n):
        for _ in range(n):
            plan.run(av, bv, out=res_c)

    def grad_calls(need_a, need_b):
        def fn(n):
            for _ in range(n):
                plan.grad(G, av, bv, need_A=need_a, need_B=need_b, out_A=gA, out_B=gB)
        return fn

    def timed(fn, n):
        sync()
        t0 = time.perf_counter()
        fn(n)
        sync()
        return (time.perf_counter() - t0) / n * 1e3  # ms per call

    kinds = [("forward", forward_calls), ("grad_A", grad_calls(True, False)), ("grad_B", grad_calls(False, True)),
             ("grad_AB", grad_calls(True, True))]
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
                     "spread_ms": round(max(r) - min(r), 5), "calls_per_block": calls[name],
                     "blocks_ms": [round(x, 5) for x in r]}
    fwd = out["forward"]["ms_median"]
    out["over_forward"] = {k: round(out[k]["ms_median"] / fwd, 3) for k in ("grad_A", "grad_B", "grad_AB")}
    out["grad_B_atomic_GBps"] = round((4.0 if f32 else 8.0) * info["kept_products"] / (out["grad_B"]["ms_median"] * 1e-3) / 1e9, 1)
    plan.close()
    if not masked:
        C.release()
    tool.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
