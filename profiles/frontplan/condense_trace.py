"""Condense a rocprofv3 kernel trace of launch_trace.py: per call (a call starts at its k_mask_* launch), in
dispatch order, one line `kernel grid workgroup lds queue` -- grid in blocks, queue numbered by first use.
With two condensed files: compare them, and the speculated calls' pre-numeric kernel counts with the timelines
under profiles/r06/timelines.
usage: condense_trace.py <run_kernel_trace.csv> > list.txt
       condense_trace.py --compare parent.txt change.txt"""
import csv
import re
import sys
from pathlib import Path

FRONT = ("k_mask_", "k_analyze", "k_probe_publish", "k_bin_list", "k_sym_", "k_near", "k_scan")
# the committed steady-state timelines (speculated calls), by the order launch_trace.py runs the stand-ins
TIMELINES = ["cant_events_off", "webbase-1M", "mac_econ_events_off", "scircuit", "cop20k_A", "cage15"]


def short(name):
    return re.sub(r"^void ", "", name.split("(")[0]).replace("mhs::", "").replace(" ", "")


def condense(path):
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))
    queues, call = {}, -1
    for r in rows:
        name = short(r["Kernel_Name"])
        if not name.startswith("k_"):
            continue  # (torch's own kernels: none between the calls)
        if name.startswith("k_mask_"):
            call += 1
            print(f"call {call}")
        wg = int(r["Workgroup_Size_X"])
        q = queues.setdefault(r["Queue_Id"], len(queues))
        print(f"  {name} grid {int(r['Grid_Size_X']) // wg} wg {wg} lds {r['LDS_Block_Size']} queue {q}")


def calls_of(path):
    calls = []
    for ln in open(path):
        if ln.startswith("call"):
            calls.append([])
        else:
            calls[-1].append(ln.split())
    return calls


def compare(pa, pb):
    a, b = calls_of(pa), calls_of(pb)
    bad = len(a) != len(b)
    print(f"calls: {len(a)} / {len(b)}")
    for i, (x, y) in enumerate(zip(a, b)):
        launches = [l[:7] for l in x] == [l[:7] for l in y]  # kernel, grid, workgroup, lds
        queues = [l[8] for l in x] == [l[8] for l in y]
        front = sum(l[0].startswith(FRONT) for l in y)
        note = ""
        if i % 2 == 1 and i // 2 < len(TIMELINES):
            f = Path(__file__).resolve().parents[1] / "r06" / "timelines" / (TIMELINES[i // 2] + ".txt")
            want = sum(any(k in ln for k in FRONT) for ln in open(f))
            note = f", {f.name}: {want} ({'same' if want == front else 'DIFFERENT'})"
            bad |= want != front
        print(f"call {i}: {len(x)} / {len(y)} kernels, launches {'equal' if launches else 'DIFFERENT'}, "
              f"queues {'equal' if queues else 'DIFFERENT'}, pre-numeric {front}{note}")
        bad |= not launches
    return 1 if bad else 0


if __name__ == "__main__":
    if sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    condense(sys.argv[1])
