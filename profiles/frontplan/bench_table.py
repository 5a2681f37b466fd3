"""Table of bench.py results of an alternation: <dir>/{default,full}_{parent,change}_<run>.json.
usage: python3 profiles/frontplan/bench_table.py <dir> <first run> <last run>"""
import json
import sys

d, lo, hi = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
runs = range(lo, hi + 1)


def load(mode, build, r):
    return json.load(open(f"{d}/{mode}_{build}_{r}.json"))


rows = [(f"headline ({m})", [[load(m, b, r)["ms_per_step"] for r in runs] for b in ("parent", "change")])
        for m in ("default", "full")]
for i, x in enumerate(load("full", "parent", lo)["configs"]["matrices"]):
    rows.append((x["matrix"], [[load("full", b, r)["configs"]["matrices"][i]["ms_per_step"] for r in runs]
                               for b in ("parent", "change")]))
print("ms per step, runs in the order they ran (parent r, change r, parent r+1, ...)")
print(f"{'figure':20s} {'parent':>{8 * len(runs)}s}   {'change':>{8 * len(runs)}s}   p.spread  c.worst-p.worst  c.median-p.median")
for name, (p, c) in rows:
    med = lambda v: sorted(v)[len(v) // 2]
    spread, worst = max(p) - min(p), max(c) - max(p)
    print(f"{name:20s} {''.join(f'{v:8.4f}' for v in p)}   {''.join(f'{v:8.4f}' for v in c)}   {spread:8.4f}  {worst:+8.4f} "
          f"{'within' if worst <= spread else 'OVER  '}  {med(c) - med(p):+8.4f}")
