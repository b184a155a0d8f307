"""CPU: the fused host finish of small fits (scaling, left-looking factorisation and forward sweep in one pass over the
statistics, 48 <= padded K <= 256) gives the bits of the separate steps it replaces -- status, coefficients, rank and
rcond estimate -- on well-conditioned systems of every padded width and remainder, on the widths next to its range, and on
every way the fast path gives up (duplicated column, NaN in G, Inf in c, zero column, small pivot)."""
import os
import subprocess
import sys

import pytest

WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host_finish_worker.py")


def run_worker(mode, variant):
    env = {k: v for k, v in os.environ.items() if not k.startswith("FSNAP_CHOL_")}
    if variant:
        env["FSNAP_CHOL_VARIANT"] = variant
    out = subprocess.run([sys.executable, WORKER, mode], capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0, out.stderr[-4000:]
    lines = out.stdout.strip().splitlines()
    assert lines and lines[-1].startswith("digest ")
    return lines


def compare(fused, legacy):
    assert len(fused) == len(legacy)
    differing = [a.rsplit(" ", 1)[0] for a, b in zip(fused, legacy) if a != b]
    assert not differing, f"fused and separate host finish differ in: {differing}"
    assert fused[-1] == legacy[-1]


@pytest.fixture(scope="module")
def outputs():
    return run_worker("cpu", None), run_worker("cpu", "3")


def test_fused_finish_has_the_bits_of_the_separate_steps(outputs):
    fused, legacy = outputs
    compare(fused, legacy)


def test_every_case_ran(outputs):
    # 20 widths x 2 families x 4 kinds, and per failure width 4 + 4 + 4 + 1 + 4 cases
    assert len(outputs[0]) == 20 * 2 * 4 + 2 * 17 + 1
    good = [l for l in outputs[0] if l.startswith("good ")]
    assert len(good) == 160
