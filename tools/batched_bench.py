#!/usr/bin/env python3
"""batched_bench.py -- one batched values call against the loop of unbatched ones, one configuration per run.

    python tools/batched_bench.py --workload {cant,scircuit,triangle} --dtype {f64,f32} --width W --batch NB
                                  [--accum f64] [--blocks 5] [--window 0.4]

(a) the loop: NB calls of mhs_spgemm_values on a width-1 plan, one per value set -- what a caller with NB value
    sets on one pattern does without the batched entry points;
(b) one mhs_spgemm_values_batched call on all NB sets through a plan of width W: ceil(NB / W) passes, each
    walking the patterns once for up to W sets.

Workloads: `cant` and `scircuit` are A*A on the product's own pattern (mhspgemm.synth.SYNTH); `triangle` is L*L on
L's pattern by a masked plan (AUTO), L the strictly lower triangle of a symmetrised synth.powerlaw graph.

Before timing every set of (b) is checked.  FP64: against (a)'s result for the set; both lie within
1.01 m 2^-53 S of the exact sum, so within twice that of each other.  FP32: against an FP64 width-1 plan on the
same rounded values, within 1.01 m 2^-24 S.  m comes from an FP64 call on all-ones; the values are positive, so S
is the FP64 result itself.  --accum f64 with --dtype f32: both plans are mixed ones (float32 values, FP64 sums); the
check is then the mixed bound against the FP64 plan, 1.01 (2^-24 |ref| + 2 m 2^-53 S) -- the mixed entry is within
2^-24 |E| + m 2^-53 S (1 + 2^-24) of the exact sum E, the FP64 one within m 2^-53 S -- and 1.01 m 2^-24 S on the
entries of global-class rows (tools/mixed_rows.py), whose sums stay float.  After warm-up the two kinds are timed in
alternating blocks as tools/values_bench.py does: a block is enough calls for its window to last `--window` seconds between device synchronisations; reported
per kind are the median of the blocks' per-call times (a call of (a) is the whole loop) and the spread (max - min).
(b) counts as faster only when it is below (a) by more than the larger spread.  The rows by class at width W and at
width 1 stand beside the times: rows move to costlier classes as the sum bytes grow.  Prints one JSON line."""
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


def lower_triangle(n: int, seed: int = 3) -> mhspgemm.CSR:
    G = synth.powerlaw(n, seed=seed)
    r = np.repeat(np.arange(G.M, dtype=np.int64), np.diff(G.ptr))
    c = G.col.astype(np.int64)
    off = r != c
    key = np.unique(np.maximum(r[off], c[off]) * n + np.minimum(r[off], c[off]))  # symmetrised, strictly lower
    ptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(key // n, minlength=n), out=ptr[1:])
    return mhspgemm.CSR(n, n, ptr.astype(np.int32), (key % n).astype(np.int32), np.ones(len(key)))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workload", default="cant", choices=("cant", "scircuit", "triangle"))
    ap.add_argument("--dtype", default="f64", choices=("f64", "f32"))
    ap.add_argument("--accum", default=None, choices=("f64",), help="with --dtype f32: FP64 sums (mixed plans)")
    ap.add_argument("--width", type=int, default=4, choices=(1, 2, 4))
    ap.add_argument("--batch", type=int, default=8, help="value sets (NB)")
    ap.add_argument("--n", type=int, default=50_000, help="vertices of the triangle workload's graph")
    ap.add_argument("--blocks", type=int, default=5, help="timed blocks per kind")
    ap.add_argument("--window", type=float, default=0.4, help="seconds a timed block should last")
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if args.batch < 1:
        ap.error("--batch: at least one value set")
    f32, W, NB = args.dtype == "f32", args.width, args.batch
    mixed = args.accum == "f64"
    if mixed and not f32:
        ap.error("--accum f64 goes with --dtype f32")
    tdt = torch.float32 if f32 else torch.float64

    dev = 0
    torch.cuda.set_device(dev)
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

    if masked:
        C, owned = A, None
    else:
        owned, _ = mhspgemm.spgemm(tool, A, A, timing=False)
        C = owned
    kw = {"masked": True, "form": "auto"} if masked else {}
    acc = {"accum": "float64"} if mixed else {}
    wide = mhspgemm.ValuesPlan(tool, A, A, C, dtype=tdt, width=W, **kw, **acc)
    one = mhspgemm.ValuesPlan(tool, A, A, C, dtype=tdt, width=1, **kw, **acc)
    iw, i1 = wide.info(), one.info()
    nC = iw["nnzC"]
    out = {"workload": args.workload, "source": source, "M": A.M, "nnzA": A.nnz, "nnzC": nC, "products": iw["products"],
           "kept_products": iw["kept_products"], "dtype": args.dtype, "accum": args.accum, "width": W, "batch": NB, "blocks": args.blocks,
           "lib": L.lib_path(), "classes": {k: iw[k] for k in mhspgemm.core.VALUES_CLASSES},
           "classes_width1": {k: i1[k] for k in mhspgemm.core.VALUES_CLASSES}}

    rng = np.random.default_rng(17)
    av = torch.from_numpy(rng.uniform(0.1, 1.0, (NB, A.nnz))).to(tdt).to(f"cuda:{dev}")
    bv = torch.from_numpy(rng.uniform(0.1, 1.0, (NB, A.nnz))).to(tdt).to(f"cuda:{dev}")
    res = torch.full((NB, nC), float("nan"), dtype=tdt, device=f"cuda:{dev}")
    loop = torch.full((NB, nC), float("nan"), dtype=tdt, device=f"cuda:{dev}")
    sync()

    def batched_call():
        wide.run_batched(av, bv, out=res)

    def loop_call():
        for b in range(NB):
            one.run(av[b], bv[b], out=loop[b])

    # ---- the check of every set
    batched_call()
    loop_call()
    ref64 = mhspgemm.ValuesPlan(tool, A, A, C, **kw)
    ones = torch.ones(A.nnz, dtype=torch.float64, device=f"cuda:{dev}")
    cnt, ref = (torch.empty(nC, dtype=torch.float64, device=f"cuda:{dev}") for _ in range(2))
    ref64.run(ones, ones, out=cnt)
    sync()
    assert not torch.isnan(res).any().item() and not torch.isnan(loop).any().item(), "an entry was not written"
    if mixed:  # the entries of the wide plan's global-class rows: C's float segment is their accumulator
        cp, cc = (np.asarray(x) for x in ((A.ptr, A.col) if masked else C.to_host()[:2]))
        rows = mixed_global_rows(cp, cc, W)
        glob = torch.from_numpy(np.repeat(rows, np.diff(cp))).to(f"cuda:{dev}")
        # (a masked plan's dot rows take precedence over the product-form rule: they may only lower the plan's count)
        assert int(rows.sum()) >= iw["global"] if masked else int(rows.sum()) == iw["global"], "the global class restated"
        out["global_rows_restated"] = int(rows.sum())
    worst = []  # per set: the largest error over its bound
    for b in range(NB):
        a64, b64 = av[b].double(), bv[b].double()
        sync()  # (torch's conversions run on its stream, the library's calls on the tool's: each waits for the other)
        ref64.run(a64, b64, out=ref)  # (positive values: S is the reference itself)
        sync()
        if mixed:
            err = (res[b].double() - ref).abs()
            bound = torch.where(glob, 1.01 * cnt * 2.0 ** -24 * ref, 1.01 * (2.0 ** -24 * ref.abs() + 2 * cnt * 2.0 ** -53 * ref))
        elif f32:
            err, bound = (res[b].double() - ref).abs(), 1.01 * cnt * 2.0 ** -24 * ref
        else:
            err, bound = (res[b] - loop[b]).abs(), 2 * 1.01 * cnt * 2.0 ** -53 * ref
        assert torch.all(res[b][cnt == 0] == 0).item(), f"set {b}: an unreached entry is not 0"
        worst.append(round(float((err[cnt > 0] / bound[cnt > 0]).max().item()) if bool((cnt > 0).any()) else 0.0, 4))
    ref64.close()
    out["checked"] = (f"every one of {NB} sets: " + ("against an FP64 width-1 plan on the same rounded values, within 1.01 (2^-24 |ref| + "
                                                      "2 m 2^-53 S), global-class rows within 1.01 m 2^-24 S" if mixed else
                                                      "against an FP64 width-1 plan on the same rounded values, within 1.01 m 2^-24 S"
                                                      if f32 else "against the unbatched call, within 2 x 1.01 m 2^-53 S"))
    out["check_worst_err_over_bound"] = worst
    out["check_pass"] = bool(max(worst) <= 1.0)
    if not out["check_pass"]:  # the figures first, then the failure
        print(json.dumps(out))
        raise SystemExit(f"check failed: worst error / bound per set {worst}")

    # ---- timing
    tool.set_option(L.MHS_OPT_SYNC, 0)

    def timed(fn, n):
        sync()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        sync()
        return (time.perf_counter() - t0) / n * 1e3  # ms per call

    kinds = [("loop", loop_call), ("batched", batched_call)]
    calls = {}
    for name, fn in kinds:
        timed(fn, args.warmup)
        per = timed(fn, 10)
        calls[name] = max(10, int(args.window * 1e3 / per) + 1)
    blocks = {name: [] for name, _ in kinds}
    for _ in range(args.blocks):
        for name, fn in kinds:
            blocks[name].append(timed(fn, calls[name]))
    tool.set_option(L.MHS_OPT_SYNC, 1)
    for name, _ in kinds:
        r = blocks[name]
        out[name] = {"ms_median": round(statistics.median(r), 5), "ms_min": round(min(r), 5), "ms_max": round(max(r), 5),
                     "spread_ms": round(max(r) - min(r), 5), "calls_per_block": calls[name],
                     "blocks_ms": [round(x, 5) for x in r]}
    spread = max(out["loop"]["spread_ms"], out["batched"]["spread_ms"])
    gain = out["loop"]["ms_median"] - out["batched"]["ms_median"]
    out["batched_vs_loop"] = {"gain_ms": round(gain, 5), "spread_ms": spread,
                              "ratio": round(out["batched"]["ms_median"] / out["loop"]["ms_median"], 4),
                              "faster_beyond_spread": bool(gain > spread), "slower_beyond_spread": bool(-gain > spread)}
    wide.close()
    one.close()
    if owned is not None:
        owned.release()
    tool.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
