"""GPU: the marginal likelihood of group-weight candidates (``fsnap_candidates_evidence``, kernels E1-E3 of
csrc/fsnap_evidence.hip; ``CandidateFits.evidence`` / ``maximise_evidence``) against the long-double oracle of
tests/candidate_evidence_cases.py at bars of 10 x what the numpy route differs from it by -- the geometry sweep, status and pivots
against the host route, batch invariance and determinism, failed candidates, the Ta golden rows, the host route beyond 144
columns, the ascent, fit() / errors() afterwards and two ranks over the peer-to-peer transport."""
import os
import subprocess
import sys

import numpy as np
import pytest

import candidate_cv_cases as cc
import candidate_evidence_cases as ec
from fitsnap_amd.config import Config
from fitsnap_amd.parallel_tools import ParallelTools
from fitsnap_amd.solvers import CandidateFits, solver_factory
from fitsnap_amd.solvers import candidates_evidence as ce

from conftest import ROOT

FIELDS = ce.FIELDS


def make_solver(name, extra=None):
    pt = ParallelTools()
    d = {"SOLVER": {"solver": name}}
    d.update(extra or {})
    return pt, solver_factory.solver(name, pt, Config(pt, d))


def candidate_fits(A, b, w0, cat, C, training):
    """``CandidateFits`` over the categorised rows of a case, its categories in the case's order."""
    keep, fs = ec.labels(cat, training)
    pt, s = make_solver("SVD")
    cf = CandidateFits(s, np.ascontiguousarray(A[keep]), b[keep], w0=w0[keep], fs_dict=fs)
    assert cf.keys == [(f"g{c // 2:02d}", not bool(training[c]), "Force" if c % 2 else "Energy") for c in range(C)]
    return pt, cf


def same_bits(x, y, rows=None):
    for name in FIELDS:
        got, want = getattr(x, name), getattr(y, name)
        assert np.array_equal(got, want if rows is None else want[rows], equal_nan=True), name


# ---------------------------------------------------------------------------------------
# 1. the sweep: every field against oracle R, status and pivots against the host route, batches as prefixes
# ---------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ec.CASES)
def test_sweep_matches_the_long_double_evidence(name):
    A, b, w0, cat, K, C, S, training = ec.case(name)
    n, _ = ec.constants(w0, cat, C)
    pt, cf = candidate_fits(A, b, w0, cat, C, training)
    for ia in range(len(cc.ALPHA_FRACTIONS)):
        alpha, ref = ec.oracle(name, ia)
        for scale in ec.SCALES:
            ev = cf.evidence(S, alpha=alpha, scale=scale, method="device")
            assert ev.method == "device" and not ev.status.any()
            k = ec.errors(ref, ev, S, alpha, n)
            print(f"{name} alpha {alpha:.2e} {scale}: " + "  ".join(f"{nm} {v:.2e}" for nm, v in zip(ec.NAMES, k))
                  + f"  min pivot {ev.min_pivot.min():.2e}")
            assert np.all(k <= ec.bars(scale)), (name, alpha, scale, dict(zip(ec.NAMES, k)))
            if alpha == 0.0:
                assert np.all(ev.grad_logalpha == 0)
        # the host route on the same blocks: the same status and live columns; a pivot is 1 - sum of < K squares of the unit-
        # diagonal scaled matrix, each rounded once, on both routes, plus the roundings of the scaling: 8 K eps
        host = cf.evidence(S, alpha=alpha, scale=scale, method="host")
        assert host.method == "host" and np.array_equal(host.status, ev.status) and np.array_equal(host.live, ev.live)
        assert np.all(np.abs(host.min_pivot - ev.min_pivot) <= 8 * K * cc.EPS), np.abs(host.min_pivot - ev.min_pivot).max()
        # batches of 1, 8 and 9 are the first candidates of the batch of 17, bit for bit
        for Pb in ec.BATCHES[:-1]:
            same_bits(cf.evidence(S[:Pb], alpha=alpha, scale=scale, method="device"), ev, slice(0, Pb))
    pt.free()


# ---------------------------------------------------------------------------------------
# 2. determinism and batch invariance
# ---------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["65", ec.C9])
def test_bits_do_not_depend_on_the_run_or_the_batch(name):
    A, b, w0, cat, K, C, S, training = ec.case(name)
    alpha = ec.case_alpha(name, 1)
    pt, cf = candidate_fits(A, b, w0, cat, C, training)
    first, second = (cf.evidence(S, alpha=alpha, method="device") for _ in range(2))
    same_bits(first, second)
    perm = np.random.default_rng(3).permutation(ec.P)
    same_bits(cf.evidence(S[perm], alpha=alpha, method="device"), first, perm)
    for p in (0, 7, 8, 16):
        same_bits(cf.evidence(S[p:p + 1], alpha=alpha, method="device"), first, slice(p, p + 1))
    pt.free()


# ---------------------------------------------------------------------------------------
# 3. device against host on the C = 9 case; auto; fit() / errors() afterwards
# ---------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_device_route_matches_the_host_route_and_leaves_everything_else_alone():
    name = ec.C9
    A, b, w0, cat, K, C, S, training = ec.case(name)
    n, _ = ec.constants(w0, cat, C)
    pt, cf = candidate_fits(A, b, w0, cat, C, training)
    betas0 = cf.fit(S)
    sums0 = cf.error_sums(betas0, S)
    layout = cf._layout
    for ia in range(len(cc.ALPHA_FRACTIONS)):
        alpha, ref = ec.oracle(name, ia)
        for scale in ec.SCALES:
            dev = cf.evidence(S, alpha=alpha, scale=scale, method="device")
            host = cf.evidence(S, alpha=alpha, scale=scale, method="host")
            auto = cf.evidence(S, alpha=alpha, scale=scale)
            assert auto.method == "device"
            same_bits(auto, dev)
            k = ec.errors(ref, dev, S, alpha, n, against=host)
            print(f"{scale} alpha {alpha:.2e}: device against host " + "  ".join(f"{nm} {v:.2e}" for nm, v in zip(ec.NAMES, k)))
            assert np.all(k <= ec.bars(scale) + ec.measured(scale))     # the sum of both routes' bars
            assert np.array_equal(dev.active, host.active) and not dev.active[:, 5].any() and not dev.active[:, 6].any()
            assert np.all(dev.grad_logS[~dev.active] == 0) and np.isnan(dev.noise[~dev.active]).all()
    # alpha=None is the solver's: 0 for SVD
    same_bits(cf.evidence(S), cf.evidence(S, alpha=0.0))
    # the layout and the statistics are untouched: a later fit() / errors() returns the bits it returned before
    assert cf._layout == layout
    assert np.array_equal(cf.fit(S), betas0) and np.array_equal(cf.error_sums(betas0, S), sums0)
    pt.free()


# ---------------------------------------------------------------------------------------
# 4. failed candidates: NaN fields for exactly them
# ---------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_duplicated_column_fails_exactly_the_candidates_that_keep_both_copies_equal():
    A, b, w0, cat, K, C, _, training = ec.case("31")
    # column 3 repeats column 2 except on the rows of category 0: a candidate that weights category 0 out has two equal columns
    A = A.copy()
    A[cat != 0, 3] = A[cat != 0, 2]
    S = 10.0 ** np.random.default_rng(8).uniform(-0.5, 0.5, (10, C))
    failing = [1, 8, 9]                                        # in the first and the second candidate tile
    S[failing, 0] = 0.0
    others = [p for p in range(10) if p not in failing]
    pt, cf = candidate_fits(A, b, w0, cat, C, training)
    for method in ("device", "host"):
        ev = cf.evidence(S, alpha=0.0, method=method)
        assert np.array_equal(np.flatnonzero(ev.status), failing), ev.status
        assert np.all(ev.min_pivot[failing] <= ce.PIVOT_TOL)
        for name in FIELDS:
            if name not in ("status", "min_pivot"):
                assert np.isnan(getattr(ev, name)[failing]).all(), name
        for name in ("log_evidence", "beta", "logdet", "grad_logS", "rss", "dof"):
            assert np.isfinite(getattr(ev, name)[others]).all(), name
        without = cf.evidence(S[others], alpha=0.0, method=method)
        assert not without.status.any()
        same_bits(without, ev, others)
    # a ridge term separates the columns again
    assert not cf.evidence(S, alpha=1e-3, method="device").status.any()
    pt.free()


# ---------------------------------------------------------------------------------------
# 5. the Ta golden rows
# ---------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(cc.TA_ALPHAS))
def test_ta_evidence_matches_the_long_double_oracle(ta, ta_fits, name):
    A, b, w0, cat, keys, S, training = ec.ta_case()
    n, _ = ec.constants(w0, cat, len(keys))
    alpha = cc.TA_ALPHAS[name]
    ref = ec.ta_oracle(name)
    pt, s = make_solver(name, {"RIDGE": {"alpha": alpha}} if name == "RIDGE" else None)
    cf = CandidateFits(s, A, b, fs_dict=cc.ta_labels(ta_fits))
    assert cf.keys == keys
    for scale in ec.SCALES:
        ev = cf.evidence(S, scale=scale)                       # alpha=None: [RIDGE] alpha, 0 for SVD
        assert ev.method == "device" and ev.alpha == alpha and not ev.status.any()
        k = ec.errors(ref, ev, S, alpha, n)
        print(f"Ta {name} {scale}: " + "  ".join(f"{nm} {v:.2e}" for nm, v in zip(ec.NAMES, k)) + f"  min pivot {ev.min_pivot.min():.2e}")
        assert np.all(k <= ec.bars(scale, ta=True)), (name, scale, dict(zip(ec.NAMES, k)))
        assert not ev.active[:, ~training].any() and ev.active[:, training].all()
    pt.free()


# ---------------------------------------------------------------------------------------
# 6. K = 145: beyond the kernels
# ---------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_k145_takes_the_host_route():
    A, b, w0, ccat, K = cc.sweep_case("145")
    cat = np.where(ccat >= 0, ccat % cc.SWEEP_C, -1).astype(np.int32)
    C, training = cc.SWEEP_C, np.ones(cc.SWEEP_C, dtype=bool)
    S = cc.sweep_scales("145")[:3]
    n, _ = ec.constants(w0, cat, C)
    pt, cf = candidate_fits(A, b, w0, cat, C, training)
    with pytest.raises(ValueError, match="144"):
        cf.evidence(S, method="device")
    ev = cf.evidence(S, method="auto")
    assert ev.method == "host" and not ev.status.any()
    k = ec.errors(ec.oracle_from(A, b, w0, cat, S, 0.0, training), ev, S, 0.0, n)
    print("K = 145 host route: " + "  ".join(f"{nm} {v:.2e}" for nm, v in zip(ec.NAMES, k)))
    assert np.all(k <= ec.bars("profiled"))
    pt.free()


# ---------------------------------------------------------------------------------------
# 7. the ascent
# ---------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_five_ascent_steps_never_lower_the_evidence():
    A, b, w0, cat, K, C, S0, training = ec.case(ec.C9)
    S0 = S0[:6]
    pt, cf = candidate_fits(A, b, w0, cat, C, training)
    S, ev, hist, conv = cf.maximise_evidence(S0, steps=5)
    print("L history:\n", hist)
    assert hist.shape == (6, 6) and np.isfinite(hist).all() and conv.shape == (6,)
    assert np.all(np.diff(hist, axis=0) >= 0) and np.any(hist[-1] > hist[0])
    assert np.array_equal(np.sign(S), np.sign(S0)) and np.all(S[:, 6] == 0)
    assert np.array_equal(S[:, 5], S0[:, 5])                   # a testing category is not stepped
    assert ev.method == "device" and np.array_equal(ev.log_evidence, hist[-1])
    same_bits(cf.evidence(S), ev)
    again = cf.maximise_evidence(S0, steps=5)
    assert np.array_equal(again[0], S) and np.array_equal(again[2], hist)
    pt.free()


# ---------------------------------------------------------------------------------------
# 8. two ranks, peer-to-peer transport, one GPU
# ---------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_two_ranks_p2p_match_one_rank(tmp_path, ta, ta_fits):
    """Both ranks return the same bits.  Against one process holding the rows in rank order they agree to rounding, not to the
    bit: the per-category blocks themselves differ, because two ranks add their chunk statistics as two partial sums and one
    addition where one process adds the chunks in sequence -- what tests/test_gpu_candidate_cv.py records for ``cross_validate``.
    Given equal blocks the evidence kernels are bit-reproducible (the determinism test above)."""
    world = 2
    procs = []
    for rank in range(world):
        env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE")}
        env.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), LOCAL_WORLD_SIZE=str(world),
                   FSNAP_COMM_FILE=str(tmp_path / "comm_id"), FSNAP_COMM_TOKEN="candidate evidence two ranks",
                   HSA_ENABLE_IPC_MODE_LEGACY="0", FSNAP_COMM_TIMEOUT="120", FSNAP_DIST_TRANSPORT="p2p")
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "candidate_evidence_dist_worker.py"), str(tmp_path)],
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=tmp_path))
    logs = []
    for p in procs:
        try:
            logs.append(p.communicate(timeout=600)[0])
        except subprocess.TimeoutExpired:
            p.kill()
            logs.append(p.communicate()[0] + "\n[killed after 600 s]")
    assert all(p.returncode == 0 for p in procs), "\n".join(logs)[-4000:]
    r0, r1 = (dict(np.load(tmp_path / f"evidence_rank{r}.npz")) for r in range(world))
    for key in r0:
        assert np.array_equal(r0[key], r1[key], equal_nan=True), key           # every rank returns the same bits
    assert not r0["status"].any()
    # one process holding the rows in rank order
    A, b, w0, cat, keys, S, training = ec.ta_case()
    n, _ = ec.constants(w0, cat, len(keys))
    alpha = cc.TA_ALPHAS["RIDGE"]
    fs_all = cc.ta_labels(ta_fits)
    order = np.concatenate([np.flatnonzero((np.arange(len(b)) // 43 % world) == r) for r in range(world)])
    fs = {k: [v[i] for i in order] for k, v in fs_all.items()}
    pt, s = make_solver("RIDGE", {"RIDGE": {"alpha": alpha}})
    cf = CandidateFits(s, np.ascontiguousarray(A[order]), np.ascontiguousarray(b[order]), fs_dict=fs)
    one = cf.evidence(S)
    two = ce.CandidateEvidence(scale="profiled", **{f: r0[f] for f in FIELDS + ("active",)})
    ref = ec.ta_oracle("RIDGE")
    kd = ec.errors(ref, two, S, alpha, n, against=one)
    ko = ec.errors(ref, two, S, alpha, n)
    print("two ranks against one process: " + "  ".join(f"{nm} {v:.2e}" for nm, v in zip(ec.NAMES, kd)))
    print("two ranks against the oracle:  " + "  ".join(f"{nm} {v:.2e}" for nm, v in zip(ec.NAMES, ko)))
    assert np.all(kd <= ec.bars("profiled", ta=True)) and np.all(ko <= ec.bars("profiled", ta=True))
    assert np.array_equal(r0["ascent_S"].shape, (3, len(keys))) and np.all(np.diff(r0["ascent_history"], axis=0) >= 0)
    pt.free()
