"""CPU: greedy sparse selection on the statistics (fsnap_omp_gram; solvers/omp_path.py's host route, picks and checks; the
``[OMP]`` config section) against the long-double yardstick and the independent checks of tests/omp_path_cases.py."""
import os
import sys

import numpy as np
import pytest

from fitsnap_amd import _capi
from fitsnap_amd.config import Config
from fitsnap_amd.solvers import lasso_path as lp
from fitsnap_amd.solvers import omp_path as op

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import omp_path_cases as cs  # noqa: E402

F = 3


def systems(seed, K):
    """The F + 1 downdated systems of the case and the total's diagonal."""
    blocks = cs.case_blocks(seed, K, F)
    folds, total = lp.sum_blocks(blocks)
    tdiag = np.ascontiguousarray(np.diag(lp.unpack(total, K)[0]))
    return [lp.downdated(folds, total, f, K)[:3] for f in range(F + 1)], tdiag


@pytest.mark.parametrize("criterion", ["omp", "ols"])
@pytest.mark.parametrize("K", [1, 2, 31, 65, 144, 200])
def test_gram_recurrence_against_the_yardstick(K, criterion):
    """S in {1, K, min(K, 128)}, every fold-left-out system and the full one: equal order, e_s and the coefficients of every
    step within the bars, every margin >= 1e-6; on the full system the supports of scikit-learn's orthogonal_mp_gram ("omp") and
    the order of brute-force forward stepwise regression on the rows ("ols")."""
    sy, tdiag = systems(100 + K, K)
    for S in sorted({1, K, min(K, 128)}):
        for f, (Qm, qv, y2) in enumerate(sy):
            order, path, coef = _capi.omp_gram(Qm, qv, y2, S, criterion, (), tdiag)
            cs.check_problem(Qm, qv, y2, tdiag, criterion, (), S, order, path, coef, where=f"K={K} S={S} {criterion} f={f}")
            assert np.all(order >= 0) and len(set(order.tolist())) == S
            assert np.all(np.diff(path[:, 0]) <= 0) and np.all(path[:, 1] >= 0) and np.all(path[:, 2] > 0)
            assert all(np.count_nonzero(coef[s]) <= s + 1 for s in range(S))
    Qm, qv, y2 = sy[F]
    order = _capi.omp_gram(Qm, qv, y2, min(K, 128), criterion, (), tdiag)[0]
    if criterion == "omp":
        sup = cs.sklearn_supports(Qm, qv, y2, min(K, 128))
        assert len(sup) == min(K, 128)
        assert all(set(order[:s + 1].tolist()) == sup[s] for s in range(len(sup)))
    else:
        A, b, w, _, _ = cs.rows(100 + K, K)
        brute = cs.stepwise_rows(A * w[:, None], b * w, min(K, 8))
        assert brute == order[:len(brute)].tolist()


@pytest.mark.parametrize("criterion", ["omp", "ols"])
def test_dead_struck_forced_columns_and_the_early_end(criterion):
    K, A, b, w, fold = cs.edge_rows(F)
    blocks = cs.blocks_ld(A, b, w, fold, F)
    folds, total = lp.sum_blocks(blocks)
    tdiag = np.ascontiguousarray(np.diag(lp.unpack(total, K)[0]))
    forced = (9, 3, 2)                    # 9 first, the dead 3 skipped without a step, then 2; its duplicate 5 is struck
    orders = []
    for f in range(F + 1):
        Qm, qv, y2, _, dead = lp.downdated(folds, total, f, K)
        order, path, coef = _capi.omp_gram(Qm, qv, y2, K, criterion, forced, tdiag)
        cs.check_problem(Qm, qv, y2, tdiag, criterion, forced, K, order, path, coef, where=f"edges {criterion} f={f}")
        orders.append(order)
        assert order[:2].tolist() == [9, 2]
        assert 3 not in order and 5 not in order and np.all(coef[:, 3] == 0.0) and np.all(coef[:, 5] == 0.0)
        assert dead[3] and dead[7] == (f == 1)
        live = K - 2 - (1 if dead[7] else 0)                 # candidates that are ever taken: not dead, not the duplicate
        assert np.all(order[:live] >= 0) and np.all(order[live:] == -1)
        assert (7 in order) == (not dead[7])
        # once the path has ended: the last e_s, zero score and pivot, the last coefficients
        assert np.all(path[live:, 0] == path[live - 1, 0]) and np.all(path[live:, 1:] == 0.0)
        assert all(np.array_equal(coef[s], coef[live - 1]) for s in range(live, K))
    assert 7 not in orders[1] and 7 in orders[0] and 7 in orders[F]
    # nothing to choose from: no step at all
    Z = np.zeros((4, 4))
    order, path, coef = _capi.omp_gram(Z, np.zeros(4), 2.5, 3, criterion)
    assert np.all(order == -1) and np.all(path == [2.5, 0.0, 0.0]) and not coef.any()
    # without diag_ref only a column with Q_jj <= 0 is dead
    Qm, qv, y2, _, _ = lp.downdated(folds, total, F, K)
    a = _capi.omp_gram(Qm, qv, y2, 4, criterion, (9,), tdiag)
    c = _capi.omp_gram(Qm, qv, y2, 4, criterion, (9,), None)
    assert all(np.array_equal(x, y) for x, y in zip(a, c))


def test_an_exact_tie_goes_to_the_lowest_index():
    Q = np.diag([4.0, 1.0, 4.0, 1.0])
    q = np.array([4.0, 1.0, 4.0, 1.0])                       # omp and ols scores: 4, 1, 4, 1
    for criterion in ("omp", "ols"):
        order, path, coef = _capi.omp_gram(Q, q, 20.0, 4, criterion)
        assert order.tolist() == [0, 2, 1, 3] and np.array_equal(path[:, 0], [16.0, 12.0, 11.0, 10.0])
        assert np.array_equal(coef[3], np.ones(4)) and np.array_equal(coef[0], [1.0, 0, 0, 0])


def test_gram_argument_errors():
    K = 4
    Q, q = np.eye(K) * 2.0, np.ones(K)
    lib = _capi.load_library()
    order, path, coef = np.zeros(K, dtype=np.int32), np.zeros((K, 3)), np.zeros((K, K))

    def status(K=K, Q=Q, q=q, ref=None, criterion=_capi.OMP_OLS, forced=(), nforced=None, S=2, outs=(order, path, coef)):
        fo = None if forced is None else np.array(list(forced) or [0], dtype=np.int32)
        return lib.fsnap_omp_gram(K, _capi._ptr(Q), _capi._ptr(q), 3.0, _capi._ptr(ref), criterion, _capi._ptr(fo),
                                  len(forced) if nforced is None else nforced, S, *(_capi._ptr(x) for x in outs))

    assert status() == _capi.OK and status(forced=(3, 1)) == _capi.OK and status(S=K) == _capi.OK
    for bad in (dict(K=0), dict(S=0), dict(S=K + 1), dict(criterion=2), dict(criterion=-1), dict(forced=(K,)), dict(forced=(-1,)),
                dict(forced=(1, 2, 1)), dict(forced=None, nforced=1), dict(forced=(), nforced=-1), dict(Q=None), dict(q=None),
                dict(outs=(None, path, coef)), dict(outs=(order, None, coef)), dict(outs=(order, path, None))):
        assert status(**bad) == _capi.E_ARG, bad
    nan = Q.copy()
    nan[1, 2] = np.nan
    assert status(Q=nan) == _capi.NUM_NONFINITE and status(ref=np.array([1.0, np.inf, 1.0, 1.0])) == _capi.NUM_NONFINITE
    # the binding turns the status into ValueError
    for kw in (dict(steps=0), dict(steps=K + 1), dict(forced=(K,)), dict(forced=(1, 1)), dict(criterion="lars")):
        with pytest.raises(ValueError):
            _capi.omp_gram(Q, q, 3.0, **{"steps": 2, **kw})


@pytest.mark.parametrize("K,S", [(31, 31), (160, 128)])
def test_host_route_on_blocks(K, S):
    """``omp_path_host`` on fold x class blocks: every problem against the yardstick (levels {1, S / 2, S}), the held-out errors
    within their bar, and nsub = 3 against the same folds summed beforehand bit for bit."""
    blocks = cs.case_blocks(300 + K, K, F, 3)
    levels = sorted({1, max(S // 2, 1), S})
    pre, total = lp.sum_blocks(blocks, 3)
    tdiag = np.diag(lp.unpack(total, K)[0])
    for criterion in ("omp", "ols"):
        out = op.omp_path_host(blocks, K, criterion, (), S, levels, nsub=3)
        one = op.omp_path_host(pre, K, criterion, (), S, levels, nsub=1, threads=1)
        assert all(np.array_equal(x, y) for x, y in zip(out, one))
        order, path, held, coef = out
        assert order.shape == (F + 1, S) and path.shape == (F + 1, S, 3) and held.shape == (F, S, 3) and coef.shape == (F + 1, 3, K)
        full = op.omp_path_host(blocks, K, criterion, (), S, np.arange(1, S + 1), nsub=3)[3]
        for f in range(F + 1):
            Qm, qv, y2, _, _ = lp.downdated(pre, total, f, K)
            at = {lv: coef[f, i] for i, lv in enumerate(levels)}
            c_ld = cs.check_problem(Qm, qv, y2, tdiag, criterion, (), S, order[f], path[f], at, where=f"host K={K} {criterion} f={f}")[3]
            if f < F:
                _, _, bb, nf = lp.unpack(pre[f], K)
                h_ld, bar = cs.heldout_ld(pre[f], K, c_ld)
                err = np.abs((np.asarray(held[f, :, 1], dtype=cs.LD) - h_ld).astype(np.float64))
                print(f"host K={K} {criterion} f={f}: held-out worst error / bar {np.max(err / bar):.3f}", flush=True)
                assert np.all(err <= bar) and np.all(held[f, :, 0] == nf) and np.all(held[f, :, 2] == bb)
                assert np.array_equal(full[f][np.array(levels) - 1], coef[f])


def test_fold_picks_on_hand_made_heldout():
    # three folds of 10 rows, four steps: pooled errors 3.0, 1.2, 1.2, 1.5 -> the tie goes to fewer terms
    sse = np.array([[10.0, 4.0, 3.0, 5.0], [10.0, 5.0, 4.0, 5.0], [10.0, 3.0, 5.0, 5.0]])
    held = np.stack([np.full((3, 4), 10.0), sse, np.full((3, 4), 20.0)], axis=2)
    terms = np.arange(1, 5)
    err, se, best, sparsest = op.cv_picks(terms, held)
    np.testing.assert_allclose(err, [1.0, 0.4, 0.4, 0.5])
    np.testing.assert_allclose(se, np.std(sse / 10.0, axis=0, ddof=1) / np.sqrt(3))
    assert best == 1 and sparsest == 1
    # one standard error of the best reaches back to fewer terms
    sse2 = sse.copy()
    sse2[:, 0] = [4.3, 5.2, 3.1]
    held2 = np.stack([np.full((3, 4), 10.0), sse2, np.full((3, 4), 20.0)], axis=2)
    err2, se2, best2, sparsest2 = op.cv_picks(terms, held2)
    assert best2 == 1 and err2[0] <= err2[1] + se2[1] and sparsest2 == 0
    # a fold without rows takes no part; no fold with rows: no pick
    held3 = np.concatenate([held, np.zeros((1, 4, 3))])
    assert op.cv_picks(terms, held3)[2:] == (1, 1)
    assert op.cv_picks(terms, np.zeros((2, 4, 3)))[2:] == (None, None)
    orders = np.array([[4, 2, 0, -1], [2, 4, 1, 3], [4, 0, 2, 1]])
    np.testing.assert_allclose(op.selection_frequency(orders, 2, 5), [1 / 3, 0, 2 / 3, 0, 1.0])
    np.testing.assert_allclose(op.selection_frequency(orders, 4, 5), [2 / 3, 2 / 3, 1.0, 1 / 3, 1.0])
    assert not op.selection_frequency(orders, None, 5).any()


def test_levels_forced_and_route_checks():
    assert op.default_levels(64).tolist() == [1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64]
    assert op.default_levels(1).tolist() == [1] and op.default_levels(5).tolist() == [1, 2, 3, 4, 5]
    assert op.default_levels(100)[-1] == 100 and np.all(np.diff(op.default_levels(100)) > 0)
    assert op.check_levels([8, 2, 2, 5], 8).tolist() == [2, 5, 8] and op.check_levels(None, 3).tolist() == [1, 2, 3]
    for bad in ([0], [9], []):
        with pytest.raises(ValueError):
            op.check_levels(bad, 8)
    assert op.check_forced((3, 1), 4).tolist() == [3, 1] and op.check_forced(None, 4).size == 0
    for bad in ((4,), (-1,), (1, 1)):
        with pytest.raises(ValueError):
            op.check_forced(bad, 4)
    with pytest.raises(ValueError):
        op.check_criterion("lars")
    assert op.choose_method("auto", 160, 64) == "host" and op.choose_method("auto", 144, 129) == "host"
    assert op.choose_method("auto", 144, 128) == "device" and op.choose_method("auto", 1, 1) == "device"
    assert op.choose_method("device", 31, 31) == "device" and op.choose_method("host", 31, 31) == "host"
    for bad in (("device", 145, 10), ("device", 144, 129), ("gpu", 10, 10)):
        with pytest.raises(ValueError):
            op.choose_method(*bad)


def test_omp_config_section():
    sec = Config(None, {"SOLVER": {"solver": "OMP"}}).sections["OMP"]
    assert (sec.terms, sec.criterion, sec.forced) == (0, "ols", ())
    sec = Config(None, {"SOLVER": {"solver": "OMP"}, "OMP": {"terms": "8", "criterion": "OMP", "forced": "3, 1,7"}}).sections["OMP"]
    assert (sec.terms, sec.criterion, sec.forced) == (8, "omp", (3, 1, 7))
    assert Config(None, {"SOLVER": {"solver": "omp"}, "OMP": {"Forced": [2, 0]}}).sections["OMP"].forced == (2, 0)
    with pytest.raises(RuntimeError, match="unmatched variable in OMP"):
        Config(None, {"SOLVER": {"solver": "OMP"}, "OMP": {"term": 3}})
    with pytest.raises(UserWarning, match="OMP section is in input"):
        Config(None, {"SOLVER": {"solver": "RIDGE"}, "OMP": {"terms": 3}})
    for bad in ({"criterion": "lars"}, {"forced": "1, 1"}, {"forced": "-2"}, {"terms": -1}):
        with pytest.raises(RuntimeError):
            Config(None, {"SOLVER": {"solver": "OMP"}, "OMP": bad})
    assert "OMP" not in Config(None, {"SOLVER": {"solver": "RIDGE"}}).sections
