"""`spgemm --subgrad N`: a modifier of --semiring NAME (not plus_times) with --reuse or --masked.  After each semiring
values line it runs N subgradient calls on seeded values and cotangents: one more line per mode and type, and with
--check the call against a sequential host loop of the rule -- ties exactly, gradients within the bound.  Without the
switch the output is what it was."""
import re
import subprocess
from pathlib import Path

import pytest

from _util import GOLDEN

ROOT = Path(__file__).resolve().parent.parent
CLI = ROOT / "mh-spgemm_amd" / "bin" / "spgemm"
MTX = str(GOLDEN / "cage4_like_A.mtx")


def run(*args, timeout=120):
    return subprocess.run([str(CLI), *args, MTX], capture_output=True, text=True, timeout=timeout)


def test_cli_subgrad_usage_errors():
    for args in (("--reuse", "2", "--subgrad", "2"),                               # no semiring to modify
                 ("--reuse", "2", "--semiring", "plus_times", "--subgrad", "2"),   # plus_times has a gradient: --grad
                 ("--semiring", "min_plus", "--subgrad", "2"),                     # no mode
                 ("--grad", "2", "--semiring", "min_plus", "--subgrad", "2"),      # --grad is not one of its modes
                 ("--reuse", "2", "--semiring", "min_plus", "--subgrad", "0"),     # no calls
                 ("--reuse", "2", "--semiring", "min_plus", "--subgrad")):         # no count
        r = run(*args, timeout=60)
        assert r.returncode == 255 and "Invalid Arguments." in r.stdout and "[--subgrad N]" in r.stdout, args
        assert "--semiring NAME" in r.stdout and "SpGEMM Start" not in r.stdout


def timing_free(out):
    """The driver's output with every number that is a time or a rate replaced."""
    return re.sub(r"\d+\.\d+", "#", out)


@pytest.mark.gpu
def test_cli_subgrad_check():
    r = run("--reuse", "2", "--masked", "2", "--semiring", "min_plus", "--subgrad", "2", "--f32", "--check")
    assert r.returncode == 0, r.stdout + r.stderr
    out = r.stdout
    for label, tag in (("values-only (pattern reused)", "values"), ("masked (A's pattern)", "masked")):
        for ty, suffix in (("FP64", ""), ("FP32", " f32")):
            m = re.search(r"^MH-SpGEMM %s min_plus subgradient %s \(both gradients\) median of 2 calls is (\d+\.\d+) ms$"
                          % (re.escape(label), ty), out, re.M)
            assert m and float(m.group(1)) > 0, out
            assert f"\n{tag} min_plus{suffix} subgrad pass\n" in out, out
            assert f"\n{tag} min_plus{suffix} pass\n" in out, out  # the mode it follows
            assert out.index(f"\n{tag} min_plus{suffix} pass\n") < out.index(f"\n{tag} min_plus{suffix} subgrad pass\n")
    assert "error" not in out and "fail" not in out.replace("failed", ""), out
    # without the switch: the same output without the added lines
    base = run("--reuse", "2", "--masked", "2", "--semiring", "min_plus", "--f32", "--check")
    assert base.returncode == 0 and "subgrad" not in base.stdout
    added = [l for l in out.splitlines() if "subgrad" in l]
    assert len(added) == 8
    assert timing_free("\n".join(l for l in out.splitlines() if "subgrad" not in l)) == timing_free("\n".join(base.stdout.splitlines()))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("max_plus", "max_min"))
def test_cli_subgrad_other_names(name):
    r = run("--masked", "1", "--semiring", name, "--subgrad", "1", "--check")
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.search(r"^MH-SpGEMM masked \(A's pattern\) %s subgradient FP64 \(both gradients\) median of 1 calls is \d+\.\d+ ms$" % name,
                     r.stdout, re.M), r.stdout
    assert f"\nmasked {name} subgrad pass\n" in r.stdout and "values " + name not in r.stdout, r.stdout
