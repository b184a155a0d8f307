"""CPU: the a-priori bars of tests/chol_cases.py are neither loose nor wrong, and the conditions tests/test_gpu_chol.py
leans on hold from the reference alone.

For every family at K in {129, 192, 257, 384, 448, 640} (3, 3, 5, 6, 7 and 10 panels: every panel count modulo 4): the
fault-free float64 mirror of the blocked algorithm stays at or below 1.0 bars (backward, forward, estimate), and on the
``gauss`` and ``spectrum1e3`` systems every applicable fault of the mirror lands more than 100 bars outside.  A failing
condition means fixing chol_cases.py's inputs or the mirror, never loosening a bar.

What the bars cannot see is said in chol_cases.py next to ``FAULTS``: a lost SECOND Newton step of a pivot reciprocal
(3e-14 relative in one row of the factor)."""
import os
import subprocess

import numpy as np
import pytest

import chol_cases as cc

FAULT_FAMILIES = ("gauss", "spectrum1e3")


def line(tag, res):
    return f"{tag}: " + " ".join(f"{k} {v:.3g}" for k, v in res.items())


def test_shapes_reach_every_panel_count_and_top_block():
    counts = {cc.panels(K) for K in cc.K_SWEEP}
    assert counts == set(range(3, 14))
    assert {cc.top_block(K) for K in cc.K_SWEEP} == {1, 2, 3, 4}
    assert {cc.top_block(K) for K in cc.K_MOD4} == {1, 2, 3, 4} and {cc.top_block(K) for K in cc.K_CPU} == {1, 2, 3}
    assert {K % 64 for K in cc.K_SWEEP} >= {0, 1, 17, 63}
    assert any(K < cc.DEVICE_MIN_K for K in cc.K_SWEEP) and cc.DEVICE_MIN_K in cc.K_SWEEP
    # factor-only form: K padded to 16 equal to and different from K padded to 64
    assert any(cc.pad(K, 16) == cc.pad(K) for K in cc.LSTSQ_K) and any(cc.pad(K, 16) != cc.pad(K) for K in cc.LSTSQ_K)


def test_probe_port_matches_the_library(tmp_path):
    """The numpy port of the probe hash against fsnap::chol_probe itself, called from a small host-compiled program."""
    from fitsnap_amd import _capi, build

    _capi.load_library()
    lib = build.lib_path()
    src = tmp_path / "probe.cpp"
    src.write_text("#include <cstdio>\nnamespace fsnap { double chol_probe(int row, int p); }\n"
                   "int main() {\n    for (int r = 0; r < 1700; ++r)\n        for (int p = 1; p <= 31; ++p) std::printf(\"%a\\n\", fsnap::chol_probe(r, p));\n"
                   "    return 0;\n}\n")
    exe = tmp_path / "probe"
    libdir = os.path.dirname(lib)
    cmd = [build._hipcc(), "-x", "c++", "-std=c++17", str(src), "-x", "none", lib, f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib",
           "-o", str(exe)]
    done = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    got = np.array([float.fromhex(t) for t in out.stdout.split()]).reshape(1700, 31)
    assert cc.same_bits(got, cc.probe_matrix(1700))
    assert np.all((np.abs(got) >= 0.25) & (np.abs(got) < 1.0)) and 0.4 < np.mean(got > 0) < 0.6


@pytest.mark.parametrize("K", cc.K_CPU)
@pytest.mark.parametrize("name", cc.ACCEPTED)
def test_mirror_within_the_bars_and_every_fault_far_outside(name, K):
    ref = cc.reference(name, K)
    assert ref.pivot >= 2.0 * cc.ACCEPT_PIVOT, ref.pivot
    got = cc.mirror(ref.G, ref.c)
    clean = cc.score(ref, got.beta, got.est)
    print(line(f"{ref.name} (pivot {ref.pivot:.3g}, lambda_min {ref.lam_min:.3g}, kappa {ref.kappa:.3g}) mirror", clean))
    assert max(clean.values()) <= 1.0, clean
    assert abs(got.pivot / ref.pivot - 1.0) <= ref.est_bar
    assert cc.in_band(ref, got.est)
    # one more right-hand side on the factor (kernel 8f's sweep)
    c2 = np.random.default_rng(K).standard_normal(K) / ref.d
    again = cc.mirror(ref.G, ref.c, rhs=c2)
    res2 = cc.score(ref, again.beta, c=c2, rhs_ref=cc.reference_rhs(ref, c2))
    print(line("    rhs", res2))
    assert max(res2.values()) <= 1.0, res2
    if name not in FAULT_FAMILIES:
        return
    faults = [f for f in cc.FAULTS if cc.applicable(K, f)]
    assert ("zero_padding" in faults) == (K % 64 != 0) and ("skip_top_offdiag" in faults) == (cc.top_block(K) in (2, 3))
    for f in faults:
        bad = cc.mirror(ref.G, ref.c, fault=f)
        hit = cc.score(ref, bad.beta)
        print(line(f"    {f}", hit))
        assert hit["bwd"] > 100.0, (f, hit)                      # the backward bar is the one every GPU case is held to


@pytest.mark.parametrize("K", cc.K_MOD4)
@pytest.mark.parametrize("alpha_rel", cc.ALPHAS)
def test_mirror_with_a_ridge_term(alpha_rel, K):
    ref = cc.reference("gauss", K, alpha_rel)
    got = cc.mirror(ref.G, ref.c, ref.alpha)
    clean = cc.score(ref, got.beta)
    print(line(f"{ref.name} (pivot {ref.pivot:.3g}) mirror", clean))
    assert max(clean.values()) <= 1.0, clean
    if alpha_rel >= 1.0e12:
        assert np.max(np.abs(ref.H - np.eye(K))) <= 1.0e-11       # H is the identity to rounding


def test_every_fault_is_applicable_somewhere():
    for f in cc.FAULTS:
        assert sum(cc.applicable(K, f) for K in cc.K_CPU) >= 2, f


# ---- what the GPU tests lean on, from the reference alone -------------------------------------------------------------------

@pytest.mark.parametrize("K", sorted(set(cc.K_MOD4 + cc.K_RHS + (cc.K_SWEEP[0], cc.K_SWEEP[-1]))))
def test_accepted_cases_clear_the_threshold_and_the_estimate_band_holds(K):
    for name in cc.ACCEPTED:
        ref = cc.reference(name, K)
        print(f"{ref.name}: pivot {ref.pivot:.3g} lambda_min {ref.lam_min:.3g} est/lambda_min {ref.est / ref.lam_min:.3g}")
        assert ref.pivot >= 2.0 * cc.ACCEPT_PIVOT, (ref.name, ref.pivot)
        assert cc.in_band(ref, ref.est), (ref.name, ref.est / ref.lam_min)
        assert ref.lam_min > 64.0 * K * cc.EPS                   # the LSTSQ kinds answer from the device factor
        # the estimate's own bar keeps the band check meaningful: est may move by far less than the band is wide
        assert ref.est_bar < 0.01


@pytest.mark.parametrize("K", cc.K_SWEEP)
def test_sweep_families_at_every_width(K):
    for name in cc.SWEEP_FAMILIES:
        ref = cc.reference(name, K)
        assert ref.pivot >= 2.0 * cc.ACCEPT_PIVOT, (ref.name, ref.pivot)
        assert cc.in_band(ref, ref.est), (ref.name, ref.est / ref.lam_min)
        assert ref.lam_min > 64.0 * K * cc.EPS


@pytest.mark.parametrize("K", cc.K_LARGE)
def test_large_widths(K):
    ref = cc.reference("gauss", K)
    print(f"{ref.name}: pivot {ref.pivot:.3g} lambda_min {ref.lam_min:.3g} est/lambda_min {ref.est / ref.lam_min:.3g}")
    assert ref.pivot >= 2.0 * cc.ACCEPT_PIVOT and cc.in_band(ref, ref.est) and ref.lam_min > 64.0 * K * cc.EPS


@pytest.mark.parametrize("K", (257, 448))
def test_refused_cases_are_below_the_threshold(K):
    for name in cc.REFUSED:
        ref = cc.reference(name, K)
        print(f"{ref.name}: pivot {ref.pivot:.3g}")
        assert ref.pivot <= 0.5 * cc.ACCEPT_PIVOT, (ref.name, ref.pivot)


def test_lstsq_rows_cases_have_a_resolvable_gram_matrix():
    for K in cc.LSTSQ_K:
        A = cc.conditioned(4 * K + 3, K, 1.0e6, "geometric", K)
        s = np.linalg.svd(A, compute_uv=False)
        assert 0.5e6 <= s[0] / s[-1] <= 2.0e6
