"""CPU test of the grouped numeric bin's cursor walk: the launch plan_numeric gives the NUM_WSG bin
and the take rule its waves follow (csrc/mhs_groupwalk.hpp) are HIP-free; tests/group_walk_check.cpp
runs them on the host as a stand-alone program under AddressSanitizer and UBSan."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def test_group_walk_under_sanitizers(tmp_path):
    exe = tmp_path / "group_walk_check"
    cc = subprocess.run(["c++", "-std=c++17", "-g", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined",
                         "-fno-sanitize-recover=all", str(ROOT / "tests" / "group_walk_check.cpp"), "-o", str(exe)],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.strip() == "group walk ok", run.stdout + run.stderr
