"""CPU: the host side of ``CandidateFits.cross_validate`` (fitsnap_amd/solvers/candidates_cv.py) and the oracles of
tests/candidate_cv_cases.py -- the host restatement of the kernels against the refit on the rows, the folds, the composed
route's scale matrix, pooling, tables, costs and argument errors.  No GPU compute is called here."""
import types

import numpy as np
import pytest

import candidate_cv_cases as cc
from fitsnap_amd.config import Config
from fitsnap_amd.parallel_tools import ParallelTools
from fitsnap_amd.solvers import CandidateFits, solver_factory
from fitsnap_amd.solvers import candidates_cv as ccv
from fitsnap_amd.solvers import lasso_path as lp


@pytest.mark.parametrize("name", cc.SWEEP_CASES)
def test_host_restatement_matches_row_oracle_within_the_recorded_measurements(name):
    A, b, w0, ccat, K = cc.sweep_case(name)
    S = cc.sweep_scales(name)
    F, C = cc.SWEEP_F, cc.SWEEP_C
    blocks = cc.blocks_numpy(A, b, w0, ccat, F * C)
    for ia in range(len(cc.ALPHA_FRACTIONS)):
        alpha, ref, ref_sums, counts, bl = cc.sweep_oracle(name, ia)
        coef, info = cc.host_cv(blocks, S, F, C, K, alpha)
        # inputs on which the reference itself never comes near the pivot rule
        assert not info[:, :, 0].any() and info[:, :, 1].min() > cc.PIVOT_FLOOR, (name, info[:, :, 1].min())
        # the recorded worst cases, with a factor 2 for the host BLAS: its summation order (and so the last bits of the
        # blocks) changes with the number of threads it runs on; the kernels' bars stay at 10 x the recorded figures
        assert cc.worst_backward(bl, S, F, C, K, alpha, coef) <= 2 * cc.MEASURED_BACKWARD
        assert cc.worst_heldout(cc.host_sums(A, b, w0, ccat, coef, F, C), ref_sums, counts, S, F) <= 2 * cc.MEASURED_HELDOUT
        assert cc.worst_forward(coef, ref) <= 2 * cc.MEASURED_FORWARD
        # live columns and the weighted training rows of the problem
        assert np.all(info[:, :, 2] == K)
        n = (S * S) @ (counts.reshape(F, C).sum(axis=0)[None, :] - counts.reshape(F, C)).T
        assert np.allclose(info[:, :, 3], n, rtol=1e-14, atol=0)


def test_row_oracle_is_the_least_squares_refit_on_the_rows():
    # the long-double normal equations against numpy.linalg.lstsq on the weighted rows themselves, at scales within a
    # decade of 1 (lstsq is the one that loses digits to wide scales)
    A, b, w0, ccat, K = cc.sweep_case("7")
    F, C = cc.SWEEP_F, cc.SWEEP_C
    S = 10.0 ** np.random.default_rng(5).uniform(-1, 1, (3, C))
    bl = cc.blocks_ld(A, b, w0, ccat, F * C)
    for alpha in (0.0, 1e-3):
        for p in range(3):
            for f in range(F):
                ref = cc.rows_lstsq(A, b, w0, ccat, S[p], f, C, alpha)
                got = np.asarray(cc.refit_ld(bl, S[p], f, F, C, K, alpha), dtype=np.float64)
                assert np.max(np.abs(got - ref)) <= 1e-11 * np.max(np.abs(ref)), (alpha, p, f)


def _fake(fs, K=3, ncat=2):
    m = len(fs["Testing"])
    return types.SimpleNamespace(fs_dict=fs, m=m, testing=np.asarray(fs["Testing"], dtype=bool), K=K, ncat=ncat,
                                 cat=(np.arange(m) % ncat).astype(np.int32), pt=types.SimpleNamespace(multi=False))


def test_folds_are_those_of_lasso_path_for_the_same_seed():
    units = [f"u{i // 3}" for i in range(60)]
    testing = [i % 11 == 0 for i in range(60)]
    cf = _fake({"Configs": units, "Testing": testing})
    for folds, seed in ((4, 0), (4, 7), (None, 0), ({f"u{i}": "ab"[i % 2] for i in range(20)}, 0)):
        ccat, fold_of_unit, F = ccv.composite_layout(cf, folds, "Configs", seed)
        trained = sorted({u for u, t in zip(units, testing) if not t})
        want, Fw = lp.deal_folds(trained, folds, seed)
        assert fold_of_unit == want and F == Fw
        for i in range(60):
            assert ccat[i] == (-1 if testing[i] else want[units[i]] * cf.ncat + cf.cat[i])
    # a row without a category of its own takes no part
    cf.cat[5] = -1
    assert ccv.composite_layout(cf, 4, "Configs", 0)[0][5] == -1


def test_composed_scale_matrix_is_zero_exactly_on_the_held_out_fold():
    S = cc.ga_scales(3, 4, 1)
    F, C = 5, 4
    Sc = ccv.composite_scales(S, F)
    assert Sc.shape == (3 * F, F * C)
    for p in range(3):
        for f in range(F):
            row = Sc[p * F + f].reshape(F, C)
            assert np.array_equal(row[f], np.zeros(C))
            for g in range(F):
                if g != f:
                    assert np.array_equal(row[g], S[p])
    sub = ccv.composite_scales(S, F, [(2, 4), (0, 1)])
    assert np.array_equal(sub[0], Sc[2 * F + 4]) and np.array_equal(sub[1], Sc[1])


def test_own_fold_keeps_each_vectors_fold():
    P, F, C = 2, 3, 2
    full = np.arange(P * F * F * C * 4, dtype=np.float64).reshape(P * F, F * C, 4)
    own = ccv.own_fold(full, P, F, C)
    for p in range(P):
        for f in range(F):
            assert np.array_equal(own[p, f * C:(f + 1) * C], full[p * F + f, f * C:(f + 1) * C])


def _hand_made():
    # two folds, four categories of which one is a testing category; two candidates
    keys = [("g0", False, "Energy"), ("g0", False, "Force"), ("g0", True, "Energy"), ("g1", False, "Energy")]
    S = np.array([[1.0, 2.0, 5.0, -3.0], [0.5, 1.0, 1.0, 1.0]])
    counts = np.array([2, 4, 0, 1, 2, 0, 0, 3])
    sums4 = np.zeros((2, 8, 4))
    sums4[0, :, :] = [[2, 4, 1, 2], [4, 8, 2, 4], [0, 0, 0, 0], [1, 1, 1, 1], [6, 12, 3, 6], [0, 0, 0, 0], [0, 0, 0, 0], [3, 9, 3, 9]]
    sums4[1] = 2 * sums4[0]
    return keys, S, counts, sums4


def test_pooling_and_tables_on_hand_made_sums():
    keys, S, counts, sums4 = _hand_made()
    pooled = ccv.pool_heldout(sums4, counts, S, 2)
    assert np.array_equal(pooled[0, 0], [4, 8, 16, 4 * 1.0, 8 * 1.0])
    assert np.array_equal(pooled[0, 1], [4, 4, 8, 2 * 2.0, 4 * 4.0])
    assert np.array_equal(pooled[0, 2], [0, 0, 0, 0, 0])
    assert np.array_equal(pooled[0, 3], [4, 4, 10, 4 * 3.0, 10 * 9.0])
    cv = ccv.CandidateCV(np.zeros((2, 2, 1)), np.zeros((2, 2), dtype=int), np.ones((2, 2)), None, {}, pooled, keys, S)
    assert cv.row_types == ["Energy", "Force"]
    index, values = cv.tables(frames=False)
    assert index == [("g0", "Energy"), ("g0", "Force"), ("g1", "Energy"), ("*ALL", "Energy"), ("*ALL", "Force")]
    assert np.allclose(values[0, 0], [4, 2.0, 2.0, 1.0, np.sqrt(2.0)])
    assert np.allclose(values[0, 3], [8, 12 / 8, np.sqrt(26 / 8), 16 / 8, np.sqrt(98 / 8)])
    frames = cv.tables()
    assert list(frames[1].columns) == ccv.COLUMNS and list(frames[1].index) == index
    assert np.array_equal(frames[1].to_numpy(), values[1])
    assert np.allclose(cv.row_type_errors[0], [[12 / 8, np.sqrt(26 / 8)], [1.0, np.sqrt(2.0)]])
    want = 2.0 * np.sqrt(26 / 8) + 0.5 * np.sqrt(2.0)
    assert np.allclose(cv.cost({"Energy": 2.0, "Force": 0.5})[0], want)
    assert np.allclose(cv.cost([2.0, 0.5], metric="rmse")[0], want)
    assert np.allclose(cv.cost({"Energy": 1.0}, metric="mae")[0], 12 / 8)
    # a category without held-out rows has NaN metrics
    assert np.isnan(ccv.metrics(np.zeros(5))[1:]).all()


def test_cost_is_nan_for_a_candidate_with_a_failed_fold():
    keys, S, counts, sums4 = _hand_made()
    pooled = ccv.pool_heldout(sums4, counts, S, 2)
    status = np.array([[0, 0], [0, 1]])
    cv = ccv.CandidateCV(np.zeros((2, 2, 1)), status, np.ones((2, 2)), None, {}, pooled, keys, S)
    cost = cv.cost({"Energy": 1.0, "Force": 1.0})
    assert np.isfinite(cost[0]) and np.isnan(cost[1])


def test_argument_errors():
    assert ccv.choose_method("auto", 144) == "auto" and ccv.choose_method("auto", 145) == "composed"
    assert ccv.choose_method("composed", 10) == "composed" and ccv.choose_method("device", 144) == "device"
    with pytest.raises(ValueError, match="144"):
        ccv.choose_method("device", 145)
    with pytest.raises(ValueError, match="method"):
        ccv.choose_method("host", 10)
    fs = {"Configs": [f"u{i // 2}" for i in range(12)], "Testing": [False] * 12}
    with pytest.raises(KeyError):
        ccv.composite_layout(_fake(fs), 3, "Structures", 0)
    with pytest.raises(ValueError, match="folds"):
        ccv.composite_layout(_fake(fs), 1, "Configs", 0)
    with pytest.raises(ValueError, match="FSNAP_CAT_STATS_MAX_BYTES"):
        ccv.composite_layout(_fake(fs, K=2000, ncat=200), 6, "Configs", 0)
    keys, S, counts, sums4 = _hand_made()
    cv = ccv.CandidateCV(np.zeros((2, 2, 1)), np.zeros((2, 2), dtype=int), np.ones((2, 2)), None, {},
                         ccv.pool_heldout(sums4, counts, S, 2), keys, S)
    with pytest.raises(ValueError, match="metric"):
        cv.cost({"Energy": 1.0}, metric="rsq")
    with pytest.raises(ValueError, match="Stress"):
        cv.cost({"Stress": 1.0})
    with pytest.raises(ValueError):
        cv.cost([1.0, 2.0, 3.0])


def test_cross_validate_refuses_before_touching_the_gpu():
    rng = np.random.default_rng(0)
    m, K = 24, 3
    fs = {"Groups": ["g"] * m, "Testing": [False] * m, "Row_Type": ["Energy", "Force"] * (m // 2)}
    pt = ParallelTools()
    s = solver_factory.solver("SVD", pt, Config(pt, {"SOLVER": {"solver": "SVD"}}))
    cf = CandidateFits(s, rng.standard_normal((m, K)), rng.standard_normal(m), fs_dict=fs)
    S = np.ones((2, cf.ncat))
    with pytest.raises(KeyError):
        cf.cross_validate(S)                                       # no Configs labels
    with pytest.raises(ValueError, match="method"):
        cf.cross_validate(S, method="rows")
    with pytest.raises(ValueError):
        cf.cross_validate(np.ones((2, cf.ncat + 1)))
    assert cf._cv is None and cf._layout is None


def test_dead_column_gets_zero_like_the_refit_on_the_rows():
    # column 2 is touched by fold 1 alone: without fold 1 no row sees it, and the minimum-norm refit gives it 0
    A, b, w0, ccat, K = cc.sweep_case("7")
    F, C = cc.SWEEP_F, cc.SWEEP_C
    A = A.copy()
    A[ccat // C != 1, 2] = 0.0
    S = cc.sweep_scales("7")[:4]
    blocks = cc.blocks_numpy(A, b, w0, ccat, F * C)
    bl = cc.blocks_ld(A, b, w0, ccat, F * C)
    coef, info = cc.host_cv(blocks, S, F, C, K, 0.0)
    assert not info[:, :, 0].any()
    assert np.array_equal(info[:, :, 2], np.tile([K, K - 1, K], (4, 1)))
    for p in range(4):
        for f in range(F):
            ref = np.asarray(cc.refit_ld(bl, S[p], f, F, C, K, 0.0), dtype=np.float64)
            assert (coef[p, f, 2] == 0.0) == (f == 1) and (ref[2] == 0.0) == (f == 1)
            assert np.max(np.abs(coef[p, f] - ref)) <= cc.FORWARD_REL * np.max(np.abs(ref)), (p, f)
    # and lstsq on the rows agrees, at scales it can resolve
    S1 = np.ones(C)
    ref = cc.rows_lstsq(A, b, w0, ccat, S1, 1, C, 0.0)
    got = cc.host_cv(blocks, S1[None, :], F, C, K, 0.0)[0][0, 1]
    assert abs(ref[2]) <= 1e-14 * np.max(np.abs(ref)) and got[2] == 0.0
    assert np.max(np.abs(got - ref)) <= 1e-11 * np.max(np.abs(ref))
