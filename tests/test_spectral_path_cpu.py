"""CPU: the host side of the grouped K-fold spectral paths -- fsnap_spectral_gram (one Jacobi eigendecomposition, then every
(alpha, rcond) setting), ``spectral_path.spectral_path_host`` over the fold frame, the picks and the statistics table -- against
the oracles of tests/spectral_path_cases.py.  No GPU is used."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

from fitsnap_amd import _capi
from fitsnap_amd.solvers import folds as ff
from fitsnap_amd.solvers import spectral_path as sp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spectral_path_cases as cs  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble


def test_header_exports_and_prototypes_stay_in_step():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fsnap_hip.h")).read(), flags=re.S)
    lib = _capi.load_library()
    nargs = {"fsnap_spectral_gram": 14, "fsnap_spectral_path": 16, "fsnap_spectral_path_times": 2}
    for name, n in nargs.items():
        decl = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, text)
        assert decl, f"{name} is not declared in fsnap_hip.h"
        assert len(decl.group(1).split(",")) == n == len(_capi.SIGNATURES[name][1]), name
        assert hasattr(lib, name) and _capi.SIGNATURES[name][0] is ctypes.c_int
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all(name in doc for name in nargs)
    assert sp.MAX_K == _capi.SPEC_MAX_K == 144


def test_every_case_is_admitted():
    """The admission is a condition on oracle B alone; every case the CPU and GPU tests use must pass it (none is skipped)."""
    for name, ns in cs.ALL_CASES:
        A, b, w, fold, cls, blocks, K, F, alphas, rconds = cs.case(name, ns)
        for f, (Qm, qv, y2, _, dead) in enumerate(cs.systems(blocks, K, ns)[2]):
            B = cs.oracle_b(Qm, qv, y2, dead, alphas, rconds)
            cs.admit(B, (name, ns, f))
            if not isinstance(name, str) and K >= 2:
                ranks = {st["rank"] for st in B["sets"]}
                assert ranks == {B["n"], B["n"] - int(np.count_nonzero(np.arange(K) % 4 == 1))}, (name, ranks)   # the tail drops


@pytest.mark.parametrize("K", cs.GRAM_K)
def test_gram_against_the_oracles(K):
    """fsnap_spectral_gram per problem (the host route) against oracle A where nothing is truncated and oracle B otherwise:
    equal ranks, n_live, supports, and every figure within 4 x the recorded worst ratio of the host route."""
    for ns in (1, 3):
        fig = cs.figures(K, ns, cs.host_route(K, ns), where="host")
        print(f"K = {K} nsub = {ns}: {fig}", flush=True)
        cs.check_bars(fig, cs.ORACLE_FACTOR, ("host", K, ns))


@pytest.mark.parametrize("name", list(cs.VARIANTS))
def test_variants_against_the_oracles(name):
    out = cs.host_route(name)
    cs.check_bars(cs.figures(name, 1, out, where="host"), cs.ORACLE_FACTOR, ("host", name), name)
    A, b, w, fold, cls, blocks, K, F, alphas, rconds = cs.case(name)
    eig, z, info, sets, fits, coef, held = out
    if name == "dup":                                       # rank K - 1 at rcond = 1e-6 and at the 4 n eps floor
        assert rconds[1] == 1e-6 and np.all(sets[:, :, 0] == K - 1)
        np.testing.assert_allclose(fits[:, 7], fits[:, 2], rtol=1e-6)      # the minimum-norm fit splits a repeated column evenly
    if name == "lone":                                      # column 5 is dead where fold 1 is held out, and only there
        assert info[1, 0] == K - 1 and np.all(info[[0, 2, 3], 0] == K)
        assert not coef[1, :, 5].any() and coef[0, :, 5].all() and fits[:, 5].all()
    if name == "empty":                                     # the fold without rows: its refit is the fit on all rows
        assert np.array_equal(coef[3], fits) and np.array_equal(eig[3], eig[4]) and not held[3].any()


def test_diagonal_identity_and_no_live_column():
    d = np.array([4.0, 1e-3, 2.5, 7.0, 1e3])
    q = np.arange(1.0, 6.0)
    r = _capi.spectral_gram(np.diag(d), q, 100.0, [0.0, 0.5], [0.0])
    assert r.sweeps == 0 and r.status == 0 and r.n_live == 5 and r.off_ratio == 0.0
    assert np.array_equal(r.eig, np.sort(d)) and np.array_equal(r.z, q[np.argsort(d)])
    np.testing.assert_allclose(r.coef[0, 0], q / d, rtol=1e-15)
    np.testing.assert_allclose(r.coef[1, 0], q / (d + 0.5), rtol=1e-15)
    np.testing.assert_allclose(r.dof[:, 0], [5.0, np.sum(d / (d + 0.5))], rtol=1e-15)
    # an identity block: repeated eigenvalues keep their positions (ties by position), one rotation for the 2 x 2 rest
    M = np.eye(6)
    M[4:, 4:] = [[2.0, 1.0], [1.0, 2.0]]
    r = _capi.spectral_gram(M, np.ones(6), 10.0, [0.0], [0.0])
    assert r.sweeps == 1 and np.allclose(r.eig, [1, 1, 1, 1, 1, 3], rtol=1e-15, atol=0) and np.all(r.rank == 6)
    np.testing.assert_allclose(r.coef[0, 0], np.linalg.solve(M, np.ones(6)), rtol=1e-14)
    # no live column: no eigenpairs, rank 0, beta = 0, sse = y2
    r = _capi.spectral_gram(np.zeros((3, 3)), np.zeros(3), 2.0, [0.0, 1.0], [0.0, 0.1])
    assert r.n_live == 0 and r.sweeps == 0 and not r.eig.any() and not r.coef.any() and not r.rank.any() and np.all(r.sse == 2.0)
    # diag_ref: a column whose diagonal the downdate left at noise is dead
    G = np.diag([1.0, 1e-12, 2.0])
    r = _capi.spectral_gram(G, np.ones(3), 5.0, [0.0], [0.0], diag_ref=np.array([1.0, 1.0, 2.0]))
    assert r.n_live == 2 and r.coef[0, 0, 1] == 0.0 and np.array_equal(r.eig, [1.0, 2.0, 0.0])
    # rcond above 1: nothing is kept
    r = _capi.spectral_gram(np.diag(d), q, 100.0, [0.0], [1.5])
    assert not r.rank.any() and not r.coef.any() and r.sse[0, 0] == 100.0 and r.dof[0, 0] == 0.0


def test_argument_checks():
    G, c = np.eye(3), np.ones(3)
    for alphas, rconds in (([-1.0], [0.0]), ([0.0], [-1e-3]), ([np.nan], [0.0]), ([0.0], [np.inf]), ([], [0.0]), ([0.0], [])):
        with pytest.raises(ValueError):
            _capi.spectral_gram(G, c, 1.0, alphas, rconds)
    with pytest.raises(ValueError):
        _capi.spectral_gram(np.eye(2), c, 1.0, [0.0], [0.0])
    bad = G.copy()
    bad[1, 2] = np.nan
    with pytest.raises(ValueError, match="infs or NaNs"):
        _capi.spectral_gram(bad, c, 1.0, [0.0], [0.0])
    lib = _capi.load_library()
    assert lib.fsnap_spectral_gram(3, None, None, 1.0, None, None, 1, None, 1, None, None, None, None, None) == _capi.E_ARG
    assert lib.fsnap_spectral_path(None, 3, 1, 1, None, None, 1, None, 1, None, None, None, None, None, None, None) == _capi.E_ARG
    for axis, name in ((sp.check_axis, "alphas"),):
        for v in ([], [-1.0], [np.nan]):
            with pytest.raises(ValueError):
                axis(v, name)
    with pytest.raises(ValueError):
        sp.choose_method("device", 145)
    assert sp.choose_method("auto", 145) == "host" and sp.choose_method("auto", 144) == "device"


def test_grid_subset_invariance():
    """Q = 1 gives the bits of its column in the wider grid, and a permuted grid the permuted bits."""
    A, b, w, fold, cls, blocks, K, F, alphas, rconds = cs.case(31)
    Qm, qv, y2, _, _ = cs.systems(blocks, K, 1)[2][1]
    wide = _capi.spectral_gram(Qm, qv, y2, alphas, rconds)
    for ia in range(len(alphas)):
        for ir in range(len(rconds)):
            one = _capi.spectral_gram(Qm, qv, y2, [alphas[ia]], [rconds[ir]])
            assert np.array_equal(one.coef[0, 0], wide.coef[ia, ir]) and one.sse[0, 0] == wide.sse[ia, ir]
            assert one.dof[0, 0] == wide.dof[ia, ir] and one.rank[0, 0] == wide.rank[ia, ir]
    perm = _capi.spectral_gram(Qm, qv, y2, alphas[::-1], rconds[::-1])
    assert np.array_equal(perm.coef[::-1, ::-1], wide.coef) and np.array_equal(perm.eig, wide.eig)


def test_host_route_against_brute_force_row_refits():
    """Each fold's rows removed and every setting solved from the remaining rows in long double: the normal equations summed
    in long double, then the Cholesky refit where nothing is truncated, and otherwise the truncated ridge solve V_kept (Lambda
    + alpha)^-1 V_kept^T c from their long-double eigendecomposition (``eig_ld``), kept: lambda > rcond^2 lambda_max -- the
    cut of ``lstsq(aw, bw, rcond)`` on the singular values."""
    K, ns = 17, 3
    A, b, w, fold, cls, blocks, _, F, alphas, rconds = cs.case(K, ns)
    eig, z, info, sets, fits, coef, held = cs.host_route(K, ns)
    Qr = len(rconds)
    for f in range(F + 1):
        rows = np.flatnonzero(fold != f)
        XL, yL = (A[rows] * w[rows, None]).astype(LD), (b[rows] * w[rows]).astype(LD)
        G, c = XL.T @ XL, XL.T @ yL
        lam, V = cs.eig_ld(G, vectors=True)
        for q in range(len(alphas) * Qr):
            alpha, rc = alphas[q // Qr], rconds[q % Qr]
            beta = fits[q] if f == F else coef[f, q]
            kept = lam > LD(cs.cut_of(rc, K, float(lam[-1])))
            assert kept.sum() == sets[f, q, 0], (f, q)
            if kept.all():
                ref = cs.chol_solve_ld(G + LD(alpha) * np.eye(K, dtype=LD), c)
            else:
                ref = V[kept].T @ ((V[kept] @ c) / (lam[kept] + LD(alpha)))
            unit = K * cs.EPS * float(lam[-1]) / (float(lam[kept].min()) + alpha)
            err = cs.scaled_err(np.asarray(G, dtype=np.float64), beta, ref)
            assert err <= cs.ORACLE_FACTOR * cs.MEASURED_COEF * unit, (f, q, err, unit)


def test_picks_and_tie_rules():
    alphas, rconds = np.array([0.0, 1.0, 2.0]), np.array([0.0, 0.1])
    #                 q:  0    1    2    3    4    5         (q = ia * 2 + ir)
    cv = np.array([3.0, 2.0, 1.0, 1.0, 1.0, 4.0])
    se = np.full(6, 0.5)
    dof = np.array([9.0, 8.0, 7.0, 6.0, 5.0, 1.0])
    best, simplest = sp.picks(alphas, rconds, cv, se, dof)
    assert best == 4                                        # ties: the larger alpha (q = 4: alpha 2) before the larger rcond
    assert simplest == 4                                    # within 1.5: q = 2, 3, 4; the smallest dof is q = 4's
    best, simplest = sp.picks(alphas, rconds, np.array([3.0, 2.0, 1.0, 1.0, 5.0, 4.0]), se, dof)
    assert best == 3 and simplest == 3                      # same alpha: the larger rcond
    best, simplest = sp.picks(alphas, rconds, np.array([1.0, 1.2, 1.4, 1.6, 5.0, 1.5]), se, dof)
    assert best == 0 and simplest == 5                      # q = 5 is within one standard error and has the smallest dof
    best, simplest = sp.picks(alphas, rconds, np.array([np.nan, 1.2, np.nan, 1.6, 5.0, np.inf]), se, dof)
    assert best == 1 and simplest == 3
    assert sp.picks(alphas, rconds, np.full(6, np.nan), se, dof) == (None, None)
    # the curve itself: folds.cv_curve over the class-summed records
    held = np.zeros((2, 2, 3, 3))
    held[..., 0] = 5.0
    held[0, :, :, 1] = [[1.0, 2.0, 3.0], [1.0, 1.0, 1.0]]
    held[1, :, :, 1] = [[3.0, 2.0, 1.0], [2.0, 2.0, 2.0]]
    folded = sp.class_sum(held)
    assert folded.shape == (2, 2, 3) and np.array_equal(folded[:, :, 0], np.full((2, 2), 15.0))
    cv_error, cv_se, _, _ = ff.cv_curve(np.zeros(2), folded)
    np.testing.assert_allclose(cv_error, [12.0 / 30.0, 9.0 / 30.0])
    np.testing.assert_allclose(cv_se, [0.0, np.std([0.2, 0.4], ddof=1) / np.sqrt(2)])


def test_stats_table_layout():
    alphas, rconds = [0.0, 1e-3], [0.0, 1e-6]
    held = np.zeros((2, 4, 3, 3))
    held[..., 0] = [4.0, 0.0, 6.0]
    held[..., 1] = np.arange(2 * 4 * 3, dtype=np.float64).reshape(2, 4, 3)
    table = sp.stats_table(alphas, rconds, held, ["Energy", "Force", "Stress"])
    assert list(table.index.names) == ["alpha", "rcond", "Row_Type"] and list(table.columns) == ["ncount", "mae", "rmse", "w_rmse"]
    assert len(table) == 4 * 4 and list(table.loc[(0.0, 1e-6)].index) == ["*ALL", "Energy", "Force", "Stress"]
    row = table.loc[(1e-3, 0.0, "Stress")]                  # q = 2, class 2: sse 8 + 20, n 12
    assert row["ncount"] == 12 and np.isnan(row["mae"]) and np.isnan(row["rmse"]) and np.isclose(row["w_rmse"], np.sqrt(28.0 / 12.0))
    empty = table.loc[(1e-3, 0.0, "Force")]
    assert empty["ncount"] == 0 and np.isnan(empty["w_rmse"])
    every = table.loc[(1e-3, 0.0, "*ALL")]                  # q = 2: sse (6 + 7 + 8) + (18 + 19 + 20), n 20
    assert every["ncount"] == 20 and np.isclose(every["w_rmse"], np.sqrt(78.0 / 20.0))
    alone = sp.stats_table(alphas, rconds, held[:, :, :1], ["Energy", "Force", "Stress"])     # folds alone: *ALL only
    assert len(alone) == 4 and set(alone.index.get_level_values(2)) == {"*ALL"}


def test_eigenvalues_are_relatively_accurate_on_a_well_scaled_case():
    """Demmel-Veselic: the diagonally scaled matrix has kappa <= 1e3, so Jacobi gives every eigenvalue -- the tail seven decades
    below the head included -- to n eps relative.  Against mpmath at 50 digits; the long-double Jacobi reference that stands in
    for mpmath at the larger sizes (``eig_ld``) is held to mpmath here, a tenth of the bar."""
    for K in (17, 31):
        A, b, w, fold, cls, blocks, _, F, alphas, rconds = cs.case(K)
        Qm = cs.well_scaled(cs.systems(blocks, K, 1)[2][F][0], np.arange(K))
        assert np.linalg.cond(Qm) >= 1e7
        ref = cs.eig_mp(Qm)
        rel = float(np.max(np.abs(cs.host_route(K)[0][F] / ref - 1.0))) / (K * cs.EPS)
        ld = float(np.max(np.abs(cs.eig_ld(Qm) / ref - 1))) / (K * cs.EPS)
        print(f"K = {K}: relative eigenvalue error {rel:.2e} n eps; eig_ld against mpmath {ld:.2e} n eps", flush=True)
        assert rel <= cs.ORACLE_FACTOR * cs.MEASURED_EIG_REL
        assert ld <= 0.1 * cs.MEASURED_EIG_REL
