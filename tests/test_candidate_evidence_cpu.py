"""CPU: the marginal likelihood of group-weight candidates (solvers/candidates_evidence.py) -- the definition against the
log density of the targets, every derivative against central differences of the long-double evidence, the numpy route against the
long-double oracle at the recorded measurements, the invariants, inactive categories, dead columns and failed candidates, the
fixed-point ascent on synthetic noise levels, the C symbol and the argument errors.  Nothing here touches a GPU."""
import os
import re

import numpy as np
import pytest

import candidate_cv_cases as cc
import candidate_evidence_cases as ec
from fitsnap_amd import _capi
from fitsnap_amd.config import Config
from fitsnap_amd.parallel_tools import ParallelTools
from fitsnap_amd.solvers import CandidateFits, solver_factory
from fitsnap_amd.solvers import candidates_evidence as ce

LD = np.longdouble
ROOT = cc.ROOT
FD_H = LD(1e-5)
FD_BAR = 1e-6            # of the largest component, the bar of tests/test_candidate_cvgrad_cpu.py: a wrong formula is off by O(1)
FD_P = 3


# ---------------------------------------------------------------------------------------
# 1. the definition: oracle R's L(fixed) is the log density of the targets
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 3, 7])
def test_fixed_scale_evidence_is_the_log_density_of_the_targets(K):
    A, b, w0, cat, s, alpha, training = ec.tiny_case(K)
    want, N = ec.density_ld(A, b, w0, cat, s, alpha, training)
    got = ec.evidence_value_ld(A, b, w0, cat, s, alpha, training)["fixed"]
    print(f"K = {K}: N = {N}, L = {float(got):.12f}, density {float(want):.12f}, difference {float(abs(got - want)):.2e}")
    assert 30 <= N <= 48
    assert float(abs(got - want)) <= 1e-12 * N
    # and the float64 route says the same
    n, slw0 = ec.constants(w0, cat, 3)
    ev = ce.host_evidence(cc.blocks_numpy(A, b, w0, cat, 3), s[None, :], alpha, n, slw0, training, K, "fixed")
    assert abs(ev.log_evidence[0] - float(want)) <= 1e-12 * N * max(1.0, abs(float(want)))


# ---------------------------------------------------------------------------------------
# 2. every derivative against central differences of the long-double evidence
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["1", "7", "31"])
def test_derivatives_match_central_differences(name):
    A, b, w0, cat, K, C, _, training = ec.case(name)
    # scales within a decade and a ridge term that matters, so that every component of the gradient is exercised
    S = 10.0 ** np.random.default_rng(5).uniform(-0.5, 0.5, (FD_P, C))
    alpha = cc.base_alpha(ec.training_blocks(A, b, w0, cat, C, training), K, 1e-2)
    ref = ec.oracle_from(A, b, w0, cat, S, alpha, training)

    def L(s, a):
        return ec.evidence_value_ld(A, b, w0, cat, s, a, training)

    for p in range(FD_P):
        s = np.asarray(S[p], dtype=LD)
        fd = {scale: np.zeros(C, dtype=LD) for scale in ec.SCALES}
        for c in range(C):
            up, dn = s.copy(), s.copy()
            up[c] *= np.exp(FD_H)
            dn[c] *= np.exp(-FD_H)
            lu, ld_ = L(up, LD(alpha)), L(dn, LD(alpha))
            for scale in ec.SCALES:
                fd[scale][c] = (lu[scale] - ld_[scale]) / (2 * FD_H)
        lu, ld_ = L(s, LD(alpha) * np.exp(FD_H)), L(s, LD(alpha) * np.exp(-FD_H))
        for scale in ec.SCALES:
            o = ref[p][scale]
            fda = (lu[scale] - ld_[scale]) / (2 * FD_H)
            big = max(float(np.max(np.abs(o["grad"]))), float(abs(o["gla"])))
            dev = max(float(np.max(np.abs(fd[scale] - o["grad"]))), float(abs(fda - o["gla"]))) / big
            print(f"K = {K} {scale} candidate {p}: deviation {dev:.2e} of the largest component {big:.2e}; "
                  f"dL/dlog alpha {float(o['gla']):.2e}")
            assert dev <= FD_BAR, (name, scale, p, dev)
            assert float(abs(o["gla"])) > 1e-3 * big           # the alpha derivative takes part in the comparison


def test_alpha_zero_derivatives_match_central_differences():
    # the restricted likelihood: N' = N - k, no log alpha term
    A, b, w0, cat, K, C, _, training = ec.case("7")
    S = 10.0 ** np.random.default_rng(6).uniform(-0.5, 0.5, (2, C))
    ref = ec.oracle_from(A, b, w0, cat, S, 0.0, training)
    for p in range(2):
        s = np.asarray(S[p], dtype=LD)
        for scale in ec.SCALES:
            fd = np.zeros(C, dtype=LD)
            for c in range(C):
                up, dn = s.copy(), s.copy()
                up[c] *= np.exp(FD_H)
                dn[c] *= np.exp(-FD_H)
                fd[c] = (ec.evidence_value_ld(A, b, w0, cat, up, 0.0, training)[scale]
                         - ec.evidence_value_ld(A, b, w0, cat, dn, 0.0, training)[scale]) / (2 * FD_H)
            o = ref[p][scale]
            big = float(np.max(np.abs(o["grad"])))
            assert float(np.max(np.abs(fd - o["grad"]))) / big <= FD_BAR, (scale, p)
            assert o["gla"] == 0


# ---------------------------------------------------------------------------------------
# 3. the numpy route against oracle R at the committed constants, and the invariants
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ec.CASES)
def test_host_route_matches_the_oracle_and_keeps_the_invariants(name):
    A, b, w0, cat, K, C, S, training = ec.case(name)
    n, _ = ec.constants(w0, cat, C)
    for ia in range(len(cc.ALPHA_FRACTIONS)):                  # alpha = 0 and alpha > 0
        alpha, ref = ec.oracle(name, ia)
        for scale in ec.SCALES:
            ev = ec.host_result(name, ia, scale)
            k = ec.errors(ref, ev, S, alpha, n)
            print(f"{name} alpha {alpha:.2e} {scale}: " + "  ".join(f"{nm} {v:.2e}" for nm, v in zip(ec.NAMES, k)))
            # the host route is what the constants were measured on: it stays within them (to the last digit printed)
            assert np.all(k <= 1.05 * ec.measured(scale)), (name, alpha, scale, k)
            assert ev.method == "host" and ev.scale == scale and not ev.status.any()
            assert np.all(ev.grad_logS[~ev.active] == 0) and np.all(ev.dof[~ev.active] == 0) and np.all(ev.rss[~ev.active] == 0)
            assert np.isnan(ev.noise[~ev.active]).all()
            if scale == "fixed":
                assert np.all(ev.sigma2 == 1)
            if ia == 0:
                assert np.all(ev.grad_logalpha == 0)
            ok = ev.active & (n[None, :] - ev.dof > 0)
            assert np.array_equal(np.isfinite(ev.noise), ok)
            assert np.allclose(ev.noise[ok], (ev.rss / (n[None, :] - ev.dof))[ok], rtol=1e-15, atol=0)


def test_inactive_categories_and_dead_columns():
    A, b, w0, cat, K, C, S, training = ec.case(ec.C9)
    ev = ec.host_result(ec.C9, 1, "profiled")
    want = (S != 0) & training[None, :]
    assert np.array_equal(ev.active, want) and not want[:, 5].any() and not want[:, 6].any() and not want[3, 2] and want[2, 2]
    # an inactive category does not enter: its scale may be anything
    S2 = S.copy()
    S2[:, 5] = 123.0
    n, slw0 = ec.constants(w0, cat, C)
    blocks = ec.training_blocks(A, b, w0, cat, C, training)
    ev2 = ce.host_evidence(blocks, S2, ev.alpha, n, slw0, training, K, "profiled")
    for name in ce.FIELDS:
        assert np.array_equal(getattr(ev, name), getattr(ev2, name), equal_nan=True), name
    A, b, w0, cat, K, C, S, training = ec.case(ec.ZERO)
    for ia in (0, 1):
        ev = ec.host_result(ec.ZERO, ia, "fixed")
        assert np.all(ev.live == K - 1) and np.all(ev.beta[:, 5] == 0) and np.isfinite(ev.log_evidence).all()


def test_failed_candidate_is_nan_and_no_other_candidate_changes():
    A, b, w0, cat, K, C, _, training = ec.case("31")
    A = A.copy()
    differ = cat == 0
    A[~differ, 3] = A[~differ, 2]                          # column 3 repeats column 2 except on the rows of category 0
    S = 10.0 ** np.random.default_rng(8).uniform(-0.5, 0.5, (4, C))
    S[1, 0] = 0.0
    n, slw0 = ec.constants(w0, cat, C)
    blocks = cc.blocks_numpy(A, b, w0, cat, C)
    ev = ce.host_evidence(blocks, S, 0.0, n, slw0, training, K)
    assert np.array_equal(ev.status, [0, 1, 0, 0]) and ev.min_pivot[1] <= ce.PIVOT_TOL
    for name in ce.FIELDS:
        if name not in ("status", "min_pivot"):
            assert np.isnan(getattr(ev, name)[1]).all(), name
    others = [0, 2, 3]
    without = ce.host_evidence(blocks, S[others], 0.0, n, slw0, training, K)
    for name in ce.FIELDS:
        assert np.array_equal(getattr(ev, name)[others], getattr(without, name)), name
    # a ridge term separates the columns again
    assert not ce.host_evidence(blocks, S, 1e-3, n, slw0, training, K).status.any()


@pytest.mark.parametrize("name", list(cc.TA_ALPHAS))
def test_ta_host_route_matches_the_oracle(name):
    A, b, w0, cat, keys, S, training = ec.ta_case()
    n, _ = ec.constants(w0, cat, len(keys))
    ref = ec.ta_oracle(name)
    for scale in ec.SCALES:
        ev = ec.ta_host(name, scale)
        k = ec.errors(ref, ev, S, cc.TA_ALPHAS[name], n)
        print(f"Ta {name} {scale}: " + "  ".join(f"{nm} {v:.2e}" for nm, v in zip(ec.NAMES, k)))
        assert np.all(k <= 1.05 * ec.measured(scale, ta=True)), (name, scale, k)
        assert not ev.active[:, ~training].any() and ev.active[:, training].all()


# ---------------------------------------------------------------------------------------
# 4. the fixed-point ascent recovers the noise levels of synthetic rows
# ---------------------------------------------------------------------------------------
NOISE_SEED = 11          # checked here on the CPU: the host route meets every assertion below with this seed


def noise_problem():
    rng = np.random.default_rng(NOISE_SEED)
    K, per = 7, 2000
    sd = np.array([1.0, 3.0, 10.0])
    cat = np.repeat(np.arange(3, dtype=np.int32), per)
    A = rng.standard_normal((3 * per, K))
    b = A @ rng.standard_normal(K) + sd[cat] * rng.standard_normal(3 * per)
    return A, b, np.ones(3 * per), cat, K, sd


@pytest.mark.parametrize("scale", ce.SCALES)
def test_fixed_point_ascent_recovers_the_noise_ratios(scale):
    """What ``maximise_evidence(method="host")`` runs: ``fixed_point`` over ``host_evidence`` (the method itself needs a context for
    the blocks)."""
    A, b, w0, cat, K, sd = noise_problem()
    n, slw0 = ec.constants(w0, cat, 3)
    blocks = cc.blocks_numpy(A, b, w0, cat, 3)
    training = np.ones(3, dtype=bool)
    S0 = np.array([[1.0, 1.0, 1.0], [0.1, -2.0, 5.0], [3.0, 0.3, 0.03], [1.0, 0.0, 1.0]])
    calls = []

    def evaluate(S):
        calls.append(S.copy())
        return ce.host_evidence(blocks, S, 0.0, n, slw0, training, K, scale)

    S, ev, hist, conv = ce.fixed_point(evaluate, S0, n, steps=50, tol=1e-6)
    print(f"{scale}: {len(hist) - 1} iterations, {len(calls)} evidence calls, 1 / |S| =\n{1 / np.abs(S[:3])}\nL = {hist[-1]}")
    assert conv.all() and hist.shape[0] <= 51
    assert np.all(np.diff(hist, axis=0) >= 0)                  # L never decreases over the accepted steps
    assert np.array_equal(ev.log_evidence, hist[-1]) and np.all(hist[-1] > hist[0])
    assert np.array_equal(np.sign(S), np.sign(S0)) and S[3, 1] == 0
    inv = 1 / np.abs(S[:3])
    # sampling error of a standard deviation from 2 000 rows: 1.6 %; 10 % is six of those
    assert np.all(np.abs(inv[:, 1] / inv[:, 0] / 3.0 - 1) <= 0.10) and np.all(np.abs(inv[:, 2] / inv[:, 0] / 10.0 - 1) <= 0.10)
    if scale == "fixed":                                       # the absolute level is identified too
        assert np.all(np.abs(inv / sd[None, :] - 1) <= 0.10)
    else:                                                      # the common scale times 1 / |S| is the noise
        assert np.all(np.abs(np.sqrt(ev.sigma2[:3, None]) * inv / sd[None, :] - 1) <= 0.10)
    # at the fixed point the noise estimate of a category is sigma^2 / S^2
    assert np.allclose(ev.noise[:3], ev.sigma2[:3, None] / S[:3] ** 2, rtol=1e-4)
    # the start without category 1 finds the other two
    assert abs(abs(S[3, 0] / S[3, 2]) / 10.0 - 1) <= 0.10


def test_fixed_point_leaves_a_nan_candidate_alone_and_is_deterministic():
    A, b, w0, cat, K, C, _, training = ec.case("31")
    A = A.copy()
    A[cat != 0, 3] = A[cat != 0, 2]
    S0 = 10.0 ** np.random.default_rng(8).uniform(-0.5, 0.5, (3, C))
    S0[1, 0] = 0.0
    n, slw0 = ec.constants(w0, cat, C)
    blocks = cc.blocks_numpy(A, b, w0, cat, C)

    def evaluate(S):
        return ce.host_evidence(blocks, S, 0.0, n, slw0, training, K)

    S, ev, hist, conv = ce.fixed_point(evaluate, S0, n, steps=5)
    assert np.array_equal(S[1], S0[1]) and np.isnan(hist[:, 1]).all() and not conv[1]
    assert np.all(np.diff(hist[:, [0, 2]], axis=0) >= 0)
    again = ce.fixed_point(evaluate, S0, n, steps=5)
    assert np.array_equal(again[0], S) and np.array_equal(again[2], hist, equal_nan=True)
    alone = ce.fixed_point(evaluate, S0[[0, 2]], n, steps=5)
    assert np.array_equal(alone[0], S[[0, 2]]) and np.array_equal(alone[2], hist[:, [0, 2]])
    zero = ce.fixed_point(evaluate, S0, n, steps=0)
    assert zero[2].shape == (1, 3) and np.array_equal(zero[0], S0)


# ---------------------------------------------------------------------------------------
# 5. the C symbol and the argument errors
# ---------------------------------------------------------------------------------------
def test_the_entry_point_is_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "fsnap_hip.h")).read()
    proto = re.search(r"int fsnap_candidates_evidence\(([^;]*)\);", header)
    assert proto and proto.group(1).count(",") + 1 == len(_capi.SIGNATURES["fsnap_candidates_evidence"][1]) == 11
    lib = _capi.load_library()
    for name in ("fsnap_candidates_evidence", "fsnap_candidates_evidence_times"):
        assert hasattr(lib, name) and name in _capi.SIGNATURES
    assert callable(getattr(_capi.HipContext, "candidates_evidence")) and callable(getattr(_capi.HipContext, "candidates_evidence_times"))
    assert '"fsnap_evidence.hip"' in open(os.path.join(ROOT, "fitsnap_amd", "build.py")).read()
    # a NULL context is refused before anything touches a GPU
    assert lib.fsnap_candidates_evidence(None, 1, 0.0, None, 1, 1, 1, None, None, None, None) == _capi.E_ARG
    assert lib.fsnap_candidates_evidence_times(None, None) == _capi.E_ARG


def test_argument_errors():
    assert ce.choose_method("auto", 144) == "device" and ce.choose_method("auto", 145) == "host"
    assert ce.choose_method("host", 10) == "host" and ce.choose_method("device", 144) == "device"
    with pytest.raises(ValueError, match="144"):
        ce.choose_method("device", 145)
    with pytest.raises(ValueError, match="method"):
        ce.choose_method("composed", 10)
    with pytest.raises(ValueError, match="scale"):
        ce.host_evidence(np.zeros((1, 5)), np.ones((1, 1)), 0.0, np.ones(1), np.zeros(1), np.ones(1, dtype=bool), 1, "free")
    for alpha in (-1.0, np.nan, np.inf):
        with pytest.raises(ValueError, match="alpha"):
            ce.host_evidence(np.zeros((1, 5)), np.ones((1, 1)), alpha, np.ones(1), np.zeros(1), np.ones(1, dtype=bool), 1)
    for bad in (dict(steps=-1), dict(tol=0.0), dict(damping=0.0), dict(damping=1.5)):
        with pytest.raises(ValueError):
            ce.fixed_point(None, np.ones((2, 2)), np.ones(2), **bad)


def test_the_methods_refuse_before_touching_the_gpu():
    rng = np.random.default_rng(0)
    m = 24
    fs = {"Groups": ["g"] * m, "Testing": [False] * m, "Row_Type": ["Energy", "Force"] * (m // 2)}
    pt = ParallelTools()
    s = solver_factory.solver("SVD", pt, Config(pt, {"SOLVER": {"solver": "SVD"}}))
    for K in (3, 145):
        cf = CandidateFits(s, rng.standard_normal((m, K)), rng.standard_normal(m), fs_dict=fs)
        S = np.ones((2, cf.ncat))
        with pytest.raises(ValueError, match="scale"):
            cf.evidence(S, scale="free")
        with pytest.raises(ValueError, match="method"):
            cf.evidence(S, method="composed")
        with pytest.raises(ValueError, match="alpha"):
            cf.evidence(S, alpha=-1.0)
        with pytest.raises(ValueError):
            cf.evidence(np.ones((2, cf.ncat + 1)))
        with pytest.raises(ValueError):
            cf.maximise_evidence(np.ones((2, cf.ncat + 1)))
        with pytest.raises(ValueError, match="method"):
            cf.maximise_evidence(S, method="composed")
        if K > ce.MAX_K:
            with pytest.raises(ValueError, match="144"):
                cf.evidence(S, method="device")
            with pytest.raises(ValueError, match="144"):
                cf.maximise_evidence(S, method="device")
        assert cf._layout is None
