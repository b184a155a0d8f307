"""CPU: the numpy yardstick of the robust (IRLS) fit, ``robust_host``, against the long-double reference of
tests/robust_cases.py; the scale semantics; the ``[ROBUST]`` section and the factory.  No GPU."""
import numpy as np
import pytest

import robust_cases as rc
from fitsnap_amd.config import Config
from fitsnap_amd.solvers import robust, solver_factory


def _host(cs, loss, **kw):
    kw.setdefault("alpha", rc.ALPHA)
    return robust.robust_host(cs.A, cs.b, cs.w, cs.mask, cs.cat, loss=loss, ncat=3, **kw)


@pytest.mark.parametrize("loss", rc.LOSSES)
@pytest.mark.parametrize("m,K", rc.SHAPES[:2])
def test_host_matches_long_double(m, K, loss):
    cs = rc.case(m, K)
    ref = rc.reference_of(m, K, loss)
    h = _host(cs, loss, max_iter=rc.FIXED_ITERS, tol=0.0)
    d = rc.distance(h.fit, ref["fit"])
    print(f"robust_host vs long double, {m} x {K}, {loss}: {d:.3e} (recorded {rc.HOST_DISTANCE[(m, K, loss)]:.1e})")
    assert h.iterations == ref["iterations"] == rc.FIXED_ITERS
    assert d <= rc.HOST_BAR
    assert d <= 10.0 * rc.HOST_DISTANCE[(m, K, loss)] + 1e-15          # the recorded figure is still the order of the day
    # per-iteration scales and tables follow the reference too: exact counts, sums to rounding
    assert np.max(np.abs(h.scales - ref["scales"].astype(float)) / ref["scales"].astype(float)) < 1e-10
    assert np.array_equal(h.tables[:, :, 0], ref["tables"][:, :, 0].astype(float))
    assert np.max(np.abs(h.tables[:, :, 3:] - ref["tables"][:, :, 3:].astype(float)) / ref["tables"][:, :, 3:].astype(float)) < 1e-9
    assert np.max(np.abs(h.omega - ref["omega"].astype(float))) < 1e-8


def test_reference_solvers_agree():
    # the wide-system form of the reference's fit (long-double gradient, fp64 preconditioner) reaches the minimiser of the
    # explicit long-double Gram + Cholesky form
    cs = rc.case(5000, 33)
    X = (np.asarray(cs.A, dtype=rc.LD) * np.asarray(cs.w, dtype=rc.LD)[:, None])[cs.part]
    y = (np.asarray(cs.b, dtype=rc.LD) * np.asarray(cs.w, dtype=rc.LD))[cs.part]
    a, b = rc.ld_ridge_explicit(X, y, rc.ALPHA), rc.ld_ridge_refined(X, y, rc.ALPHA)
    assert rc.distance(b, a) < 1e-17


@pytest.mark.parametrize("loss", rc.LOSSES)
def test_closed_forms(loss):
    # r and rho of the yardstick against the long-double closed forms (scalar and vectorised), around the branch points
    c = rc.DEFAULT_TUNE[loss]
    s = np.array([0.5, 2.0, 0.0, 1e-3])
    u = np.array([0.0, 1e-9, 0.5, 1.0, -1.0, c * (1 - 1e-12), c, c * (1 + 1e-12), -2 * c, 10.0, -300.0, 1e8])
    e = (u[:, None] * np.where(s > 0, s, 1.0)[None, :]).ravel()
    sv = np.tile(s, len(u))
    r, rho = robust.robust_weight(loss, c, sv, e)
    r1, rho1 = rc.ref_weight(loss, c, sv, e)
    r2, rho2 = rc.ref_weight_vec(loss, c, sv, e)
    assert np.array_equal(r1, r2) and np.array_equal(rho1, rho2)
    assert np.max(np.abs(r - r1.astype(float))) <= 4 * rc.EPS
    assert np.max(np.abs(rho - rho1.astype(float)) / np.maximum(1.0, np.abs(rho1.astype(float)))) <= 8 * rc.EPS
    zero = sv == 0.0
    assert np.all(r[zero] == 1.0) and np.all(rho[zero] == 0.0)
    # the branch is decided on |e| against the single product c * s
    inside = np.abs(e) <= c * sv if loss == "huber" else np.abs(e) < c * sv
    if loss == "huber":
        assert np.all(r[inside & ~zero] == 1.0) and np.all(r[~inside & ~zero] <= 1.0)
    if loss == "bisquare":
        assert np.all(r[~inside & ~zero] == 0.0) and np.all(r[inside & ~zero] > 0.0)
    # omega = psi(u) / u: r^2 u reproduces the derivative of rho
    ok = ~zero & (np.abs(e) > 0) & (np.abs(e / np.where(zero, 1, sv)) < 1e3)
    uu = (e / np.where(zero, 1.0, sv))[ok].astype(rc.LD)
    h = rc.LD(1e-7) * np.maximum(1, np.abs(uu))
    num = (rc.ref_weight_vec(loss, c, 1.0, uu + h)[1] - rc.ref_weight_vec(loss, c, 1.0, uu - h)[1]) / (2 * h)
    away = np.abs(np.abs(uu) - c) > 1e-3 if loss != "cauchy" else np.ones(len(uu), dtype=bool)
    assert np.max(np.abs(num - (r1[ok] ** 2) * uu)[away] / np.maximum(1, np.abs(uu[away]))) < 1e-6


def test_outlier_benefit():
    cs = rc.case(3000, 17)
    part = cs.part
    ls = np.linalg.lstsq((cs.A * cs.w[:, None])[part], (cs.b * cs.w)[part], rcond=None)[0]
    err_ls = np.max(np.abs(ls - cs.truth))
    planted = cs.outliers[part[cs.outliers]]
    assert len(planted) > 100
    for loss in rc.LOSSES:
        h = _host(cs, loss)
        assert h.converged
        ratio = np.max(np.abs(h.fit - cs.truth)) / err_ls
        print(f"{loss}: max |beta - truth| = {ratio:.3f} x least squares, largest omega of a planted outlier "
              f"{h.omega[planted].max():.3f}")
        assert ratio <= 0.2
        assert np.all(h.omega[planted] < 0.5)
        assert np.all(h.omega[~part] == 1.0)


def test_scale_semantics():
    # class sizes 1, 2, 3, an even count with ties, a class whose median is exactly 0, an empty class; test rows and
    # zero-weight rows carry huge residuals that must not reach a median
    sizes = {0: 1, 1: 2, 2: 3, 3: 6, 4: 7}                  # class 5 stays empty
    vals = {0: [3.0], 1: [1.0, -4.0], 2: [5.0, -1.0, 2.0], 3: [2.0, 2.0, -2.0, 7.0, 7.0, 0.5], 4: [0.0, 0.0, 0.0, 0.0, 9.0, -3.0, 1.0]}
    cat = np.concatenate([[g] * n for g, n in sizes.items()] + [[0, 1, 2, 3, 4, 5], [0, 1, 2, 3, 4, 5]])
    e = np.concatenate([vals[g] for g in sizes] + [[1e9] * 6, [1e9] * 6])
    m = len(e)
    mask = np.ones(m, dtype=bool)
    mask[-12:-6] = False                                    # test rows
    w = np.ones(m)
    w[-6:] = 0.0                                            # zero-weight rows
    part = mask & (w > 0)
    s, n = robust.class_scales(e, cat, 6, part)
    assert n.tolist() == [1, 2, 3, 6, 7, 0]
    assert s.tolist() == [1.4826 * 3.0, 1.4826 * ((1.0 + 4.0) * 0.5), 1.4826 * 2.0, 1.4826 * ((2.0 + 2.0) * 0.5), 0.0, 0.0]
    assert np.all(np.abs(s - rc.ref_scales(e[part], cat[part], 6).astype(float)) <= 2 * rc.EPS * s)   # (one fp64 product)
    # the whole iteration on rows that produce exactly these residuals from beta = 0: A = 0 columns would be singular, so one
    # column of ones in a class of its own keeps the fit alive; classes with s = 0 or no rows get r = 1
    for loss in rc.LOSSES:
        r, rho = robust.robust_weight(loss, rc.DEFAULT_TUNE[loss], s[cat], e)
        assert np.all(r[cat >= 4] == 1.0) and np.all(rho[cat >= 4] == 0.0)
    A = np.ones((m, 1))
    h = robust.robust_host(A, e, w, mask, cat, loss="huber", ncat=6, start=np.zeros(1), max_iter=1, alpha=0.0)
    assert np.array_equal(h.scales[0], s)
    assert h.tables[0, :, 0].tolist() == [1, 2, 3, 6, 7, 0]
    assert np.all(h.omega[~part] == 1.0)
    assert np.all(h.omega[(cat == 4) & part] == 1.0)


def test_convergence_scale_iters_and_fixed_scale():
    cs = rc.case(3000, 17)
    h = _host(cs, "huber", tol=1e-8)
    assert h.converged and 3 <= h.iterations <= 40
    ref = rc.reference(cs.A, cs.b, cs.w, cs.mask, cs.cat, 3, "huber", max_iter=50, tol=1e-8)
    assert ref["converged"] and abs(ref["iterations"] - h.iterations) <= 1
    assert rc.distance(h.fit, ref["fit"]) < 1e-7
    # max_iter reached without convergence
    h2 = _host(cs, "huber", tol=1e-14, max_iter=2)
    assert not h2.converged and h2.iterations == 2
    # scale_iters: the scales of iteration 3 on stay those of iteration 2
    h3 = _host(cs, "bisquare", tol=0.0, max_iter=6, scale_iters=3)
    assert np.array_equal(h3.scales[3], h3.scales[2]) and np.array_equal(h3.scales[5], h3.scales[2])
    assert not np.array_equal(h3.scales[1], h3.scales[2])
    r3 = rc.reference(cs.A, cs.b, cs.w, cs.mask, cs.cat, 3, "bisquare", max_iter=6, scale_iters=3)
    assert rc.distance(h3.fit, r3["fit"]) <= rc.HOST_BAR
    # a fixed scale replaces the MAD entirely
    fixed = np.array([0.1, 0.05, 0.02])
    h4 = _host(cs, "cauchy", tol=0.0, max_iter=6, scale=fixed)
    assert np.all(h4.scales == fixed[None, :])
    r4 = rc.reference(cs.A, cs.b, cs.w, cs.mask, cs.cat, 3, "cauchy", max_iter=6, scale=fixed)
    assert rc.distance(h4.fit, r4["fit"]) <= rc.HOST_BAR
    with pytest.raises(ValueError):
        _host(cs, "lad")
    with pytest.raises(ValueError):
        _host(cs, "huber", tune=0.0)


def test_robust_section_defaults_and_rejected_keys():
    cfg = Config(None, {"SOLVER": {"solver": "ROBUST"}})
    sec = cfg.sections["ROBUST"]
    assert (sec.loss, sec.tune, sec.alpha, sec.scale_by, sec.scale_iters, sec.max_iter, sec.tol) == \
        ("huber", None, 1.0e-8, "row_type", 0, 50, 1.0e-8)
    cfg = Config(None, {"SOLVER": {"solver": "ROBUST"}, "ROBUST": {"loss": "Bisquare", "tune": "4.0", "scale_by": "Groups+Row_Type",
                                                                   "scale_iters": 3, "max_iter": "20", "tol": 1e-6, "alpha": 1e-6}})
    sec = cfg.sections["ROBUST"]
    assert (sec.loss, sec.tune, sec.alpha, sec.scale_by, sec.scale_iters, sec.max_iter, sec.tol) == \
        ("bisquare", 4.0, 1e-6, "groups+row_type", 3, 20, 1e-6)
    with pytest.raises(RuntimeError, match="unmatched variable in ROBUST"):
        Config(None, {"SOLVER": {"solver": "ROBUST"}, "ROBUST": {"looss": "huber"}})
    with pytest.raises(UserWarning):
        Config(None, {"SOLVER": {"solver": "RIDGE"}, "ROBUST": {"loss": "huber"}})
    assert robust.resolve_loss("CAUCHY", None) == ("cauchy", 2.385)
    assert robust.DEFAULT_TUNE == rc.DEFAULT_TUNE


def test_torch_distributed_group_is_refused_before_anything_runs():
    from types import SimpleNamespace

    solver = SimpleNamespace(pt=SimpleNamespace(multi=True, comm_kind="torch"))
    with pytest.raises(NotImplementedError, match="native transports"):
        robust.robust_fit(solver)


def test_factory_finds_robust():
    assert solver_factory.search("ROBUST").__class__ is robust.ROBUST
    assert solver_factory.search("robust").__class__ is robust.ROBUST
