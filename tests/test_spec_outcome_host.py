"""CPU test of what becomes of a speculated call after the hand-off: spec_outcome (csrc/mhs_shape.hpp) against
its table on the host under sanitizers.  The GPU tests of tests/test_gpu_spec_duress.py reach the table's rows
on the device; that they would notice the rows the earlier expression got wrong is shown here."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def test_spec_outcome_under_sanitizers(tmp_path):
    # all 16 combinations of (spec, launched, err, same) against literals: tests/spec_outcome_check.cpp, HIP-free
    exe = tmp_path / "spec_outcome_check"
    cc = subprocess.run(["c++", "-std=c++17", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                         "-fno-sanitize-recover=all", str(ROOT / "tests" / "spec_outcome_check.cpp"), "-o", str(exe)],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.strip() == "spec outcome ok", run.stdout + run.stderr
