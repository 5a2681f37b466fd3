"""CPU checks of the edge ladder (tests/test_gpu_edges.py runs it on the GPU).

tests/shape_edges.cpp derives, from csrc/mhs_shape.hpp and csrc/mhs_valplan.hpp alone, the last row parameter that
stays in a bin or class and the first that leaves it; its output is committed as tests/golden/shape_edges.json.
Here: the fixture still equals what the program prints (built with -Wall -Werror under AddressSanitizer and UBSan,
so a changed constant cannot leave the rungs behind), and the generators of tests/_util.py put every copy of every
rung's row exactly on the fixture's parameters, both sides of the edge -- recomputed from the matrices and the
oracle's C, not from the generators' own arithmetic."""
import json
import subprocess
from pathlib import Path

import numpy as np
import pytest

from oracle import oracle as orc
from _util import EDGE_COPIES, GOLDEN, edge_case, edge_rows, load_edges, row_shapes

ROOT = Path(__file__).resolve().parent.parent
EDGES = load_edges()
FULL = [(g, r["name"], side) for g in ("numeric", "dense", "symbolic") for r in EDGES[g] for side in ("last", "first")]
VALUES = [(r["name"], side) for r in EDGES["values"] for side in ("last", "first")]


def rung(group, name):
    return next(r for r in EDGES[group] if r["name"] == name)


def test_fixture_equals_helper_under_sanitizers(tmp_path):
    exe = tmp_path / "shape_edges"
    cc = subprocess.run(["c++", "-std=c++17", "-g", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined",
                         "-fno-sanitize-recover=all", "-I", str(ROOT / "mh-spgemm_amd" / "csrc"),
                         str(ROOT / "tests" / "shape_edges.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and not run.stderr, run.stderr
    json.loads(run.stdout)
    assert run.stdout == (GOLDEN / "shape_edges.json").read_text(), \
        "tests/golden/shape_edges.json is not what tests/shape_edges.cpp prints from the headers: regenerate it"


def test_row_classification_ends_on_any_ints(tmp_path):
    """tests/shape_total_check.cpp: the functions k_scan classifies a row with return on hostile tile and entry
    counts -- what a row of a left-out symbolic launch holds (next_pow2 did not, above 2^30: the kernel hung)."""
    exe = tmp_path / "shape_total_check"
    cc = subprocess.run(["c++", "-std=c++17", "-O0", "-Wall", "-Werror", "-I", str(ROOT / "mh-spgemm_amd" / "csrc"),
                         str(ROOT / "tests" / "shape_total_check.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=20)
    assert run.returncode == 0 and run.stdout.startswith("2000 calls"), (run.stdout, run.stderr)


def test_every_rung_of_the_ladder_is_there():
    names = {g: [r["name"] for r in EDGES[g]] for g in ("numeric", "dense", "symbolic", "values")}
    assert (len(names["numeric"]), len(names["dense"]), len(names["symbolic"]), len(names["values"])) == (18, 4, 7, 9)
    for g, ns in names.items():
        assert len(set(ns)) == len(ns), g
    for g in ("numeric", "symbolic"):
        for r in EDGES[g]:
            bin_key = {"num": "num_bin", "sym": "sym_bin"}.get(r["count"])
            if bin_key and not r["name"].startswith("stage"):  # a step from one bin into another (stage rungs: within one)
                assert r["last"][bin_key] != r["first"][bin_key], r["name"]
    for r in EDGES["values"]:
        assert r["last"]["class"] != r["first"]["class"], r["name"]


@pytest.mark.parametrize("group,name,side", FULL)
def test_rung_rows_sit_on_their_edge(group, name, side):
    r = rung(group, name)
    A, B = edge_case(r["family"], r[side]["params"], r["R"])
    assert A[0] == EDGE_COPIES * r["R"]
    Cp, Ci, _ = orc.spgemm(A[2], A[3], A[4], B[2], B[3], B[4], B[1])
    got = row_shapes(A, B, Cp, Ci)
    for k, want in r[side]["row"].items():
        assert np.all(got[k] == want), (k, want, got[k])
    assert r[side]["row"]["flop"] > 512 or r[side]["row"]["nA"] > 64, "outside the tiny classes"
    # the copies differ in pattern (R equal rows in a row are one group): no further row groups form
    rows = [tuple(A[3][A[2][i]:A[2][i + 1]]) for i in range(A[0])]
    assert len(set(rows)) == EDGE_COPIES and all(rows[i] == rows[i - i % r["R"]] for i in range(A[0]))
    assert set(np.abs(A[4]).tolist()) | set(np.abs(B[4]).tolist()) <= {1.0, 2.0, 3.0}


@pytest.mark.parametrize("name,side", VALUES)
def test_values_rung_rows_sit_on_their_edge(name, side):
    p = rung("values", name)[side]["params"]
    A, B = edge_case("val", p)
    Cp, Ci, _ = orc.spgemm(A[2], A[3], A[4], B[2], B[3], B[4], B[1])
    got = row_shapes(A, B, Cp, Ci)
    assert A[0] == EDGE_COPIES
    assert np.all(got["n"] == p["n"]) and np.all(got["colspan"] == p["span"]) and np.all(got["flop"] == p["products"])


def test_row_count_matrix_shape():
    A, B = edge_rows(1025)
    Cp, Ci, _ = orc.spgemm(A[2], A[3], A[4], B[2], B[3], B[4], B[1])
    got = row_shapes(A, B, Cp, Ci)
    assert A[0] == 1025 and sorted(set(got["nA"].tolist())) == [2, 201]
    assert np.count_nonzero(got["nA"] == 201) == 4 and np.all(got["n"] == got["flop"])
