"""The calls whose launches profiles/frontplan compares between two builds: every BASELINE stand-in twice on
one context (the second call speculates on the first's plan), then scircuit-like twice on a context with
MHS_SYM_FORK=1.  Run under `rocprofv3 --kernel-trace --output-format csv -d DIR -o run -- python3
profiles/frontplan/launch_trace.py [--lib DIR]`; prints one JSON line per call with the context's counters.
usage: python3 profiles/frontplan/launch_trace.py [--lib DIR] [matrix ...]"""
import argparse
import json
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(ROOT), str(ROOT / "mh-spgemm_amd")]
ap = argparse.ArgumentParser()
ap.add_argument("matrices", nargs="*", default=["cant", "webbase-1M", "mac_econ_fwd500", "scircuit", "cop20k_A", "cage15"])
ap.add_argument("--lib", default=None)
args = ap.parse_args()
if args.lib:
    os.environ["MHS_LIB"] = str(Path(args.lib).resolve() / "libmhspgemm.so")
import torch  # noqa: E402,F401
import mhspgemm  # noqa: E402
from mhspgemm import synth  # noqa: E402

COUNTERS = ["spec", "spec_miss", "spec_skipped", "sym_fork", "nft", "near", "multi_stream", "split", "chunked"]


def two_calls(tool, name, label):
    A, _ = synth.load_or_synth(name)
    A.H2D(0)
    for call in range(2):
        C, t = mhspgemm.spgemm(tool, A, A)
        C.release()
        print(json.dumps({"matrix": label, "call": call, "rows": A.M, "nnzC": int(t.nnzC),
                          **{k: tool.stat(k) for k in COUNTERS}}), flush=True)
    A.d_release_csr()


tool = mhspgemm.Tool(0)
for name in args.matrices:
    two_calls(tool, name, name)
tool.close()
os.environ["MHS_SYM_FORK"] = "1"  # (read when a context is created)
tool = mhspgemm.Tool(0)
two_calls(tool, "scircuit", "scircuit MHS_SYM_FORK=1")
tool.close()
