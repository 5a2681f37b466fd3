#!/usr/bin/env python3
"""values_bench.py -- the repeated full call against the values-only call, one config per run.

    python tools/values_bench.py [--config cant] [--blocks 5] [--window 0.4] [--full-only] [--dtype f32|f64] [--accum f64]
                                 [--semiring plus_times|min_plus|max_plus|max_min]

(a) the repeated full call, timed as bench.py times its steps: mhs_spgemm on one pair of
    operands, speculation on, MHS_OPT_SYNC 0 on torch's current stream, each C handed back to
    the pool before the next call;
(b) mhs_spgemm_values through a ValuesPlan on C's pattern, on value arrays other than the ones
    the pattern came from (two sets, alternating), into C's own val.

Before timing, (b)'s output is checked against the full product of the same new operands:
pattern equal, values by the reference 1e-9 rule.  After warm-up the two are timed in
alternating blocks; a block is enough calls for its window to last `--window` seconds, between a
host clock read after a device synchronise and one after the next.  Reported per kind: the median
of the blocks' per-call times and the spread (max - min) between blocks of that kind.  (b) counts
as faster only when it is below (a) by more than the larger spread.

--dtype f32 runs (b) through an FP32 plan on float32 values.  Its check is then against an FP64 plan on the same
rounded values: every entry within 1.01 m 2^-24 S, m and S from the FP64 plan on all-ones and on absolute
values; the FP64 plan's rows by class are reported beside the FP32 plan's (`classes_f64`).

--accum f64 with --dtype f32 runs (b) through a mixed plan: float32 values, FP64 sums (ValuesPlan(..., accum="float64")).
Its check is against the FP64 plan on the same rounded values too, at the mixed plan's bound: with E the exact sum the
mixed entry is within 2^-24 |E| + m 2^-53 S (1 + 2^-24) of it and the FP64 one within m 2^-53 S, so every entry is
within 1.01 (2^-24 |ref| + 2 m 2^-53 S) of the FP64 plan's; the entries of global-class rows (more than 13,312 entries
over more than 19,968 columns: C's float segment is their accumulator) within the FP32 bound.  The mixed plan's rows by
class (`classes`) are the FP64 plan's (`classes_f64`), which the run asserts.

--semiring NAME (default plus_times) runs (b) through a plan of that semiring, of either --dtype, on the same
values.  Its check is then an equality: every entry against a sequential reduce of the products in the plan's
dtype (index arithmetic and scatter_reduce in torch, A's entries a slice at a time).  The JSON line carries the
name as `semiring` and is otherwise the one of the plus-times run.

--full-only times (a) alone and needs nothing of the values-only entry points, so it also runs
against an older library (MHS_LIB=/path/to/libmhspgemm.so).  Prints one JSON line."""
from __future__ import annotations

import argparse
import json
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


def semiring_reference(name, A, Cptr, Ccol, av, bv, chunk=1 << 24):
    """C's values of A (x) A under `name` on the pattern (Cptr, Ccol): every product av[p] (x) bv[q] reduced into its
    slot, about `chunk` products at a time.  av, bv: device tensors of one dtype; the result has it."""
    dev = av.device
    Ap, Ac = (torch.from_numpy(np.asarray(x, np.int64)).to(dev) for x in (A.ptr, A.col))
    Cp, Cc = (torch.from_numpy(np.asarray(x, np.int64)).to(dev) for x in (Cptr, Ccol))
    N = int(A.N)
    rowA = torch.repeat_interleave(torch.arange(A.M, device=dev), Ap[1:] - Ap[:-1])
    keyC = torch.repeat_interleave(torch.arange(A.M, device=dev), Cp[1:] - Cp[:-1]) * N + Cc
    lens = Ap[Ac + 1] - Ap[Ac]
    ends = torch.cumsum(lens, 0)
    identity = float("inf") if name == "min_plus" else float("-inf")
    out = torch.full((len(Ccol),), identity, dtype=av.dtype, device=dev)
    a0 = 0
    while a0 < len(Ac):
        done = int(ends[a0 - 1]) if a0 else 0
        a1 = max(a0 + 1, int(torch.searchsorted(ends, torch.tensor(done + chunk, device=dev), right=True)))
        n = lens[a0:a1]
        p = torch.repeat_interleave(torch.arange(a0, a1, device=dev), n)
        start = ends[a0:a1] - n - done
        q = Ap[Ac[p]] + torch.arange(len(p), device=dev) - torch.repeat_interleave(start, n)
        slot = torch.searchsorted(keyC, rowA[p] * N + Ac[q])
        prod = torch.minimum(av[p], bv[q]) if name == "max_min" else av[p] + bv[q]
        out.scatter_reduce_(0, slot, prod, "amin" if name == "min_plus" else "amax", include_self=True)
        a0 = a1
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", default="cant", help="a BASELINE matrix name (mhspgemm.synth.SYNTH); default cant")
    ap.add_argument("--blocks", type=int, default=5, help="timed blocks per kind")
    ap.add_argument("--window", type=float, default=0.4, help="seconds a timed block should last")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--full-only", action="store_true", help="time the repeated full call alone")
    ap.add_argument("--dtype", default="f64", choices=("f32", "f64"), help="the values plan's value type")
    ap.add_argument("--accum", default=None, choices=("f64",), help="with --dtype f32: FP64 sums (a mixed plan)")
    ap.add_argument("--semiring", default="plus_times", choices=tuple(getattr(mhspgemm.core, "SEMIRINGS", {"plus_times": 0})),
                    help="the values plan's semiring")
    args = ap.parse_args()
    f32 = args.dtype == "f32"
    semiring = args.semiring != "plus_times"
    mixed = args.accum == "f64"
    if mixed and (not f32 or semiring):
        ap.error("--accum f64 goes with --dtype f32 and the plus_times semiring")

    dev = 0
    torch.cuda.set_device(dev)
    A, source = synth.load_or_synth(args.config)
    flop = mhspgemm.flop_count_np(A.col, A.ptr)
    A.H2D(dev)
    tool = mhspgemm.Tool(dev)
    tool.set_stream(torch.cuda.current_stream(dev).cuda_stream)

    def sync():
        torch.cuda.synchronize(dev)

    out = {"config": args.config, "source": source, "M": A.M, "nnzA": A.nnz, "flop": int(flop), "blocks": args.blocks,
           "lib": L.lib_path(), "dtype": args.dtype, "semiring": args.semiring, "accum": args.accum}

    # ---- the pattern, and (b)'s check against the full product of the same new operands
    C, _ = mhspgemm.spgemm(tool, A, A, timing=False)
    out["nnzC"] = C.nnz
    plan = None
    vals = []
    res32 = None
    if not args.full_only and semiring:
        tdtype = torch.float32 if f32 else torch.float64
        plan = mhspgemm.ValuesPlan(tool, A, A, C, dtype="float32" if f32 else "float64", semiring=args.semiring)
        info = plan.info()
        out["classes"] = {k: info[k] for k in mhspgemm.core.VALUES_CLASSES}
        out["plan_bytes"] = info["plan_bytes"]
        rng = np.random.default_rng(17)
        for _ in range(2):
            vals.append(tuple(torch.from_numpy(rng.uniform(0.1, 1.0, A.nnz)).to(f"cuda:{dev}").to(tdtype) for _ in range(2)))
        res32 = torch.full((C.nnz,), float("nan"), dtype=tdtype, device=f"cuda:{dev}")  # (the output of either dtype)
        sync()
        p0, c0, _ = C.to_host()
        for av, bv in vals:
            plan.run(av, bv, out=res32)
            sync()
            assert torch.equal(res32, semiring_reference(args.semiring, A, p0, c0, av, bv)), "not the sequential reduce"
        out["checked"] = "equal to a sequential reduce of the products in the plan's dtype (2 value sets)"
    elif not args.full_only and f32:
        plan = mhspgemm.ValuesPlan(tool, A, A, C, dtype="float32", **({"accum": "float64"} if mixed else {}))
        info = plan.info()
        out["classes"] = {k: info[k] for k in mhspgemm.core.VALUES_CLASSES}
        out["plan_bytes"] = info["plan_bytes"]
        rng = np.random.default_rng(17)
        for _ in range(2):
            vals.append(tuple(torch.from_numpy(rng.uniform(0.1, 1.0, A.nnz).astype(np.float32)).to(f"cuda:{dev}")
                              for _ in range(2)))
        res32 = torch.full((C.nnz,), float("nan"), dtype=torch.float32, device=f"cuda:{dev}")
        ref, cnt = (torch.empty(C.nnz, dtype=torch.float64, device=f"cuda:{dev}") for _ in range(2))
        ones = torch.ones(A.nnz, dtype=torch.float64, device=f"cuda:{dev}")
        sync()
        plan64 = mhspgemm.ValuesPlan(tool, A, A, C)
        i64 = plan64.info()
        out["classes_f64"] = {k: i64[k] for k in mhspgemm.core.VALUES_CLASSES}
        plan64.run(ones, ones, out=cnt)
        glob = None
        if mixed:  # the entries of global-class rows, by the plan header's rule at 8 sum bytes
            assert out["classes"] == out["classes_f64"], "a mixed plan's rows by class are the FP64 plan's"
            p0, c0, _ = C.to_host()
            rows = mixed_global_rows(p0, c0, 1)
            assert int(rows.sum()) == info["global"], "the global class restated"
            glob = torch.from_numpy(np.repeat(rows, np.diff(p0))).to(f"cuda:{dev}")
        for av, bv in vals:
            plan64.run(av.double(), bv.double(), out=ref)  # (positive values: S is the reference itself)
            plan.run(av, bv, out=res32)
            sync()
            assert not torch.isnan(res32).any().item(), "an entry was not written"
            f32_bound = 1.01 * cnt * 2.0 ** -24 * ref
            if mixed:
                bound = torch.where(glob, f32_bound, 1.01 * (2.0 ** -24 * ref.abs() + 2 * cnt * 2.0 ** -53 * ref))
                assert torch.all((res32.double() - ref).abs() <= bound).item(), "outside 2^-24 |ref| + 2 m 2^-53 S"
            else:
                assert torch.all((res32.double() - ref).abs() <= f32_bound).item(), "outside m 2^-24 S"
        plan64.close()
        out["checked"] = ("against an FP64 plan on the same rounded values: every entry within 1.01 (2^-24 |ref| + 2 m 2^-53 S), "
                          "global-class rows within 1.01 m 2^-24 S (2 value sets)" if mixed else
                          "against an FP64 plan on the same rounded values: every entry within 1.01 m 2^-24 S (2 value sets)")
    elif not args.full_only:
        plan = mhspgemm.ValuesPlan(tool, A, A, C)
        info = plan.info()
        out["classes"] = {k: info[k] for k in mhspgemm.core.VALUES_CLASSES}
        out["plan_bytes"] = info["plan_bytes"]
        rng = np.random.default_rng(17)
        for _ in range(2):  # two sets of new values for A's and B's roles
            vals.append(tuple(torch.from_numpy(rng.uniform(0.1, 1.0, A.nnz)).to(f"cuda:{dev}") for _ in range(2)))
        sync()
        p0, c0, _ = C.to_host()
        for av, bv in vals:
            A1 = mhspgemm.CSR(A.M, A.N, A.ptr, A.col, av.cpu().numpy())
            B1 = mhspgemm.CSR(A.M, A.N, A.ptr, A.col, bv.cpu().numpy())
            A1.H2D(dev)
            B1.H2D(dev)
            F, _ = mhspgemm.spgemm(tool, A1, B1, timing=False)
            fp, fc, fv = F.to_host()
            F.release()
            plan.run(av, bv)
            sync()
            _, _, gv = C.to_host()
            assert np.array_equal(fp, p0) and np.array_equal(fc, c0), "pattern of the full product changed"
            assert mhspgemm.compare_ref(fp, fc, fv, p0, c0, gv), "values outside the reference 1e-9 rule"
        out["checked"] = "pattern equal, values within the reference 1e-9 rule (2 value sets)"

    # ---- timing
    tool.set_option(L.MHS_OPT_SYNC, 0)
    state = {"C": None}

    def full_calls(n):
        for _ in range(n):
            if state["C"] is not None:
                state["C"].release()
            state["C"], _ = mhspgemm.spgemm(tool, A, A, timing=False)

    def values_calls(n):
        for i in range(n):
            av, bv = vals[i & 1]
            plan.run(av, bv, out=res32)  # (FP64: out None, C's own val)

    def timed(fn, n):
        sync()
        t0 = time.perf_counter()
        fn(n)
        sync()
        return (time.perf_counter() - t0) / n * 1e3  # ms per call

    kinds = [("full", full_calls)] + ([] if args.full_only else [("values", values_calls)])
    calls = {}
    for name, fn in kinds:
        fn(args.warmup)
        per = timed(fn, 20)
        calls[name] = max(20, int(args.window * 1e3 / per) + 1)
    res = {name: [] for name, _ in kinds}
    for _ in range(args.blocks):
        for name, fn in kinds:
            res[name].append(timed(fn, calls[name]))
    tool.set_option(L.MHS_OPT_SYNC, 1)
    for name, _ in kinds:
        r = res[name]
        out[name] = {"ms_median": round(statistics.median(r), 5), "ms_min": round(min(r), 5), "ms_max": round(max(r), 5),
                     "spread_ms": round(max(r) - min(r), 5), "calls_per_block": calls[name],
                     "gflops_median": round(2.0 * flop / (statistics.median(r) * 1e6), 2),
                     "blocks_ms": [round(x, 5) for x in r]}
    if not args.full_only:
        spread = max(out["full"]["spread_ms"], out["values"]["spread_ms"])
        gain = out["full"]["ms_median"] - out["values"]["ms_median"]
        out["values_vs_full"] = {"gain_ms": round(gain, 5), "spread_ms": spread, "ratio": round(
            out["values"]["ms_median"] / out["full"]["ms_median"], 4), "faster_beyond_spread": bool(gain > spread)}
    if state["C"] is not None:
        state["C"].release()
    if plan is not None:
        plan.close()
    C.release()
    tool.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
