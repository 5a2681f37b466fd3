"""`spgemm --smooth lse [--softgrad N]`: modifiers of --semiring min_plus | max_plus with --reuse or --masked.  After
the semiring lines each mode runs once more on a smoothed plan (log-sum-exp), then N soft gradient calls: one more line
each per mode and type, and with --check both against a sequential host loop in long double at the header's bounds.
Without the switches the output is what it was."""
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


def test_cli_smooth_usage_errors():
    for args in (("--reuse", "2", "--smooth", "lse"),                                               # no semiring to smooth
                 ("--reuse", "2", "--semiring", "plus_times", "--smooth", "lse"),                   # a sum is smooth already
                 ("--reuse", "2", "--semiring", "max_min", "--smooth", "lse"),                      # no smoothed max-min
                 ("--semiring", "min_plus", "--smooth", "lse"),                                     # no mode
                 ("--reuse", "2", "--semiring", "min_plus", "--smooth", "softmax"),                 # not a smoothing
                 ("--reuse", "2", "--semiring", "min_plus", "--smooth"),                            # no word
                 ("--reuse", "2", "--semiring", "min_plus", "--softgrad", "2"),                     # nothing smoothed
                 ("--reuse", "2", "--semiring", "min_plus", "--smooth", "lse", "--softgrad", "0"),  # no calls
                 ("--reuse", "2", "--semiring", "min_plus", "--smooth", "lse", "--softgrad")):      # no count
        r = run(*args, timeout=60)
        assert r.returncode == 255 and "Invalid Arguments." in r.stdout, args
        assert "[--smooth lse] [--softgrad N]" in r.stdout and "SpGEMM Start" not in r.stdout


def timing_free(out):
    """The driver's output with every number that is a time or a rate replaced."""
    return re.sub(r"\d+\.\d+", "#", out)


@pytest.mark.gpu
def test_cli_smooth_check():
    r = run("--reuse", "2", "--masked", "2", "--semiring", "min_plus", "--smooth", "lse", "--softgrad", "2", "--f32", "--check")
    assert r.returncode == 0, r.stdout + r.stderr
    out = r.stdout
    for label, tag in (("values-only (pattern reused)", "values"), ("masked (A's pattern)", "masked")):
        for ty, suffix in (("FP64", ""), ("FP32", " f32")):
            m = re.search(r"^MH-SpGEMM %s min_plus lse %s median of 2 calls is (\d+\.\d+) ms$" % (re.escape(label), ty), out, re.M)
            assert m and float(m.group(1)) > 0, out
            m = re.search(r"^MH-SpGEMM %s min_plus lse gradient %s \(both gradients\) median of 2 calls is (\d+\.\d+) ms$"
                          % (re.escape(label), ty), out, re.M)
            assert m and float(m.group(1)) > 0, out
            assert f"\n{tag} min_plus{suffix} lse pass\n" in out, out
            assert f"\n{tag} min_plus{suffix} softgrad pass\n" in out, out
            assert out.index(f"\n{tag} min_plus{suffix} pass\n") < out.index(f"\n{tag} min_plus{suffix} lse pass\n") \
                < out.index(f"\n{tag} min_plus{suffix} softgrad pass\n")
    assert "error" not in out and "fail" not in out.replace("failed", ""), out
    # without the switches: the same output without the added lines
    base = run("--reuse", "2", "--masked", "2", "--semiring", "min_plus", "--f32", "--check")
    assert base.returncode == 0 and " lse" not in base.stdout and "softgrad" not in base.stdout
    added = [l for l in out.splitlines() if " lse" in l or "softgrad" in l]
    assert len(added) == 16
    assert timing_free("\n".join(l for l in out.splitlines() if l not in added)) == timing_free("\n".join(base.stdout.splitlines()))


@pytest.mark.gpu
def test_cli_smooth_max_plus_forward_only():
    r = run("--masked", "1", "--semiring", "max_plus", "--smooth", "lse", "--check")
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.search(r"^MH-SpGEMM masked \(A's pattern\) max_plus lse FP64 median of 1 calls is \d+\.\d+ ms$", r.stdout, re.M), r.stdout
    assert "\nmasked max_plus lse pass\n" in r.stdout and "softgrad" not in r.stdout and "gradient" not in r.stdout, r.stdout
