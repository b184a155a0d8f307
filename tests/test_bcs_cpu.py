"""CPU: the BCS recurrence on the statistics (fsnap_bcs_gram) against the reference's own ``bcs()`` (tests/golden/
bcs_reference.npz) and against the direct posterior in long double, its edges and argument rules, the ``[BCS]`` section, the
BCS solver through the factory and the host route of ``bcs_path`` (cases, references and bars: tests/bcs_cases.py).
No GPU compute is called here."""
import os
import sys

import numpy as np
import pytest

from fitsnap_amd import _capi
from fitsnap_amd.config import Config
from fitsnap_amd.parallel_tools import ParallelTools
from fitsnap_amd.solvers import ard_path as ap
from fitsnap_amd.solvers import bcs_path as bp
from fitsnap_amd.solvers import folds as ff
from fitsnap_amd.solvers import solver_factory

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bcs_cases as cs  # noqa: E402

ETA = 1e-18
PICK_TAGS = ["ta", "ta_testing", "ta_transpose", "k2", "k7", "k33", "k144", "k7_del", "k33_del"]    # more than one candidate


def gram_of(tag, ta, **kw):
    Q, q, y2, sum_y, n = cs.case_statistics(tag, ta)
    args = dict(eta=ETA, itermax=10, scale=0.01)
    args.update(kw)
    return (Q, q, y2, sum_y, n), _capi.bcs_gram(Q, q, y2, sum_y, n, **args)


def test_goldens_are_the_recorded_constructions():
    g = cs.golden()
    dels = {t: int(g[f"{t}_deletions"]) for t in cs.tags()}
    assert sum(1 for d in dels.values() if d > 0) >= 2 and sum(1 for d in dels.values() if d == 0) >= 2
    assert dels["k7_del"] > 0 and dels["k33_del"] > 0
    assert sorted(g[f"{t}_A"].shape[1] for t in cs.tags() if f"{t}_A" in g) == [1, 2, 7, 7, 33, 33, 144]
    for t in cs.tags():
        if f"{t}_args" in g:
            m, K, c, nnz, noise, seed = g[f"{t}_args"]
            assert m <= 400
            A, y = cs.synthetic(int(m), int(K), float(c), int(nnz), float(noise), int(seed))
            np.testing.assert_allclose(A, g[f"{t}_A"], rtol=1e-12, atol=1e-12)
            np.testing.assert_allclose(y, g[f"{t}_y"], rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("tag", cs.tags())
def test_reference_mode_against_the_reference(ta, tag):
    """Same ``used`` in order; coefficients, errbars and the clipped Sig within 1e-8 of their largest entry, sigma2 within 1e-8
    (measured: <= 2e-10 / 3e-9 / 5e-9 / 7e-10, the Ta rows being the worst)."""
    want = cs.expected(tag)
    _, r = gram_of(tag, ta)
    assert r.status in (0, 2)
    assert r.active.tolist() == want["used"].tolist()
    dw, de = cs.rel(r.mu, want["weights"]), cs.rel(r.errbars, want["errbars"])
    dS = cs.rel(np.maximum(r.Sig, 0.0), want["Sig"])
    ds = abs(r.sigma2 - float(want["sigma2"])) / float(want["sigma2"])
    print(f"{tag}: weights {dw:.2e} errbars {de:.2e} Sig {dS:.2e} sigma2 {ds:.2e} margin {r.margin:.3e}", flush=True)
    assert dw < cs.REF_BAR and de < cs.REF_BAR and dS < cs.REF_BAR and ds < cs.REF_BAR
    assert np.array_equal(r.coef[r.active], r.mu) and np.count_nonzero(r.coef) == r.active.size
    assert (int(want["deletions"]) > 0) == bool((r.picks[:, 1] == _capi.BCS_DEL).any())


@pytest.mark.parametrize("tag", PICK_TAGS)
def test_every_case_used_for_picks_has_a_margin(ta, tag):
    for deletion in ("reference", "exact"):
        _, r = gram_of(tag, ta, deletion=deletion)
        print(f"{tag} {deletion}: margin {r.margin:.3e}", flush=True)
        assert r.margin >= cs.MIN_MARGIN, (tag, deletion, r.margin)


@pytest.mark.parametrize("name", list(cs.PATH_CASES))
def test_every_path_case_has_a_margin(name):
    info = cs.case_host(name)[5]
    print(f"{name}: smallest margin {info[:, :, 5].min():.3e}", flush=True)
    assert info[:, :, 5].min() >= cs.MIN_MARGIN
    assert not (info[:, :, 1] == 1).any()


def posterior_gap(stats, r):
    Q, q = stats[0], stats[1]
    mu, Sig = cs.posterior_ld(Q, q, r.active, r.alpha, r.sigma2_in)
    return cs.rel(r.mu, mu.astype(np.float64)), cs.rel(r.Sig, Sig.astype(np.float64))


@pytest.mark.parametrize("tag", ["k1", "k2", "k7", "k33", "k144", "k7_del", "k33_del"])
def test_exact_mode_is_the_direct_posterior(ta, tag):
    """(active, alpha, sigma2_in) of an "exact" run, and of any run without a deletion, give mu and Sig of the direct posterior
    to 1e-10; a "reference" run that went through a deletion does not: the switch does something."""
    had_deletion = int(cs.expected(tag)["deletions"]) > 0
    stats, ex = gram_of(tag, ta, deletion="exact")
    dm, dS = posterior_gap(stats, ex)
    print(f"{tag} exact: mu {dm:.2e} Sig {dS:.2e}", flush=True)
    assert dm < cs.POSTERIOR_BAR and dS < cs.POSTERIOR_BAR
    _, ref = gram_of(tag, ta, deletion="reference")
    dm, dS = posterior_gap(stats, ref)
    print(f"{tag} reference: mu {dm:.2e} Sig {dS:.2e}", flush=True)
    if had_deletion:
        assert dm > 1e3 * cs.POSTERIOR_BAR           # mu, S and Q are stale after the reference's deletion
    else:
        assert dm < cs.POSTERIOR_BAR and dS < cs.POSTERIOR_BAR
        assert np.array_equal(ref.picks, ex.picks) and np.array_equal(ref.mu, ex.mu)


def small(K=6, m=80, seed=5):
    A, y = cs.synthetic(m, K, 1.0, 2, 0.3, seed)
    return cs.statistics_ld(A, y)


def test_edges():
    # K = 1: the one column, re-estimated; nothing else can be chosen and the margin stays inf
    Q, q, y2, sy, n = small(1)
    r = _capi.bcs_gram(Q, q, y2, sy, n, itermax=4)
    assert r.active.tolist() == [0] and r.margin == np.inf and set(r.picks[:r.iterations, 1]) <= {_capi.BCS_RE, _capi.BCS_STOP}
    # a dead column from diag_ref: never chosen although it carries the signal; diag_ref = 0 kills too
    Q, q, y2, sy, n = small(6)
    free = _capi.bcs_gram(Q, q, y2, sy, n)
    lead = int(free.active[0])
    ref = np.diag(Q).copy()
    ref[lead] = Q[lead, lead] * 1e11
    dead = _capi.bcs_gram(Q, q, y2, sy, n, diag_ref=ref)
    assert lead not in dead.active and dead.coef[lead] == 0.0 and lead not in dead.picks[:, 0]
    ref[lead] = 0.0
    assert lead not in _capi.bcs_gram(Q, q, y2, sy, n, diag_ref=ref).active
    none = _capi.bcs_gram(Q, q, y2, sy, n, diag_ref=np.zeros(6))
    assert none.active.size == 0 and none.iterations == 0 and none.status == 0 and not none.coef.any()
    assert np.all(none.picks == -1) and none.rss == y2
    # the full set blocks additions
    for ma in (1, 2):
        r = _capi.bcs_gram(Q, q, y2, sy, n, max_active=ma, itermax=12)
        adds = int((r.picks[:, 1] == _capi.BCS_ADD).sum())
        assert r.active.size <= ma and adds <= ma - 1 + int((r.picks[:, 1] == _capi.BCS_DEL).sum())
        assert r.Sig.shape == (r.active.size, r.active.size)
    assert _capi.bcs_gram(Q, q, y2, sy, n, max_active=2, itermax=12).active.size == 2
    # eta = 1: the test is first looked at in the third iteration and holds there
    r = _capi.bcs_gram(Q, q, y2, sy, n, eta=1.0)
    assert r.iterations == 3 and r.status == 0 and r.picks[2, 1] == _capi.BCS_STOP and np.all(r.picks[3:] == -1)
    # itermax = 1
    r = _capi.bcs_gram(Q, q, y2, sy, n, itermax=1)
    assert r.iterations == 1 and r.status == 2 and r.picks.shape == (1, 2) and r.active.size in (1, 2)
    # sigma2 given, and the reference's rule
    var = y2 / n - (sy / n) ** 2
    assert _capi.bcs_gram(Q, q, y2, sy, n).sigma2_in == max(0.01 * var, 1e-16)
    assert _capi.bcs_gram(Q, q, y2, sy, n, scale=0.5).sigma2_in == max(0.5 * var, 1e-16)
    assert _capi.bcs_gram(Q, q, y2, sy, n, sigma2=0.125).sigma2_in == 0.125
    # a lone column that the noise swamps (sigma2 above its ratio) starts from a negative alpha and a negative Sig: the
    # reference's determinant assertion is status 1 here, with NaN coefficients and no exception
    Q1, q1 = np.array([[4.0]]), np.array([0.02])
    r = _capi.bcs_gram(Q1, q1, 1.0, 0.0, 10.0, sigma2=1.0)
    assert r.status == 1 and np.isnan(r.coef).all() and r.alpha[0] < 0.0 and r.active.tolist() == [0]


def test_degenerate_starts():
    """"No column has a finite ml at the first step".  While a column is active it always scores (a re-estimate or a deletion,
    and a NaN score wins the argmax), so the "no candidate" end inside the loop is a guard that only a formula returning -inf
    could reach; the inputs that come closest are worked out here by hand.  One live column beside a dead one (Q_00 = 2,
    q_0 = 1, sigma2 = 1/4): ratio 1/2, alpha = 2 / (1/2 - 1/4) = 8, Sig = 1 / (8 + 8) = 1/16, mu = 1/4; alpha is at its optimum, so
    every iteration re-estimates column 0 and changes nothing, to itermax.  With sigma2 = 5 above the ratio alpha starts at
    2 / (1/2 - 5) = -4/9 and Sig = 1 / (-4/9 + 2/5) < 0: theta <= 0 asks for a deletion with one column left, which ends the
    problem at its first iteration, and the negative Sig is status 1 with NaN coefficients.  (All columns dead: test_edges.)"""
    Q = np.array([[2.0, 0.0], [0.0, 0.0]])
    q = np.array([1.0, 0.0])
    ref = np.array([2.0, 1.0])              # column 1 is dead by diag_ref
    r = _capi.bcs_gram(Q, q, 1.0, 0.0, 4.0, sigma2=0.25, diag_ref=ref, itermax=6)
    assert r.active.tolist() == [0] and r.status == 2 and r.iterations == 6 and r.picks.tolist() == [[0, _capi.BCS_RE]] * 6
    assert abs(r.alpha[0] - 8.0) < 1e-12 and abs(r.mu[0] - 0.25) < 1e-14 and abs(r.Sig[0, 0] - 1.0 / 16.0) < 1e-15
    assert r.coef.tolist() == [r.mu[0], 0.0] and r.margin == np.inf
    r = _capi.bcs_gram(Q, q, 1.0, 0.0, 4.0, sigma2=5.0, diag_ref=ref, itermax=6)
    assert r.status == 1 and r.iterations == 1 and r.picks[0].tolist() == [0, _capi.BCS_STOP] and np.all(r.picks[1:] == -1)
    assert abs(r.alpha[0] + 4.0 / 9.0) < 1e-14 and r.Sig[0, 0] < 0.0 and np.isnan(r.coef).all() and r.active.tolist() == [0]


def test_nan_in_the_statistics_and_argument_rules():
    Q, q, y2, sy, n = small(4)
    for bad in (dict(Q=np.where(np.eye(4) > 0, np.nan, Q)), dict(q=q * np.inf), dict(y2=np.nan), dict(sum_y=np.inf), dict(n=np.nan),
                dict(diag_ref=np.array([1.0, np.nan, 1.0, 1.0]))):
        kw = dict(Q=Q, q=q, y2=y2, sum_y=sy, n=n)
        kw.update(bad)
        with pytest.raises(ValueError, match="infs or NaNs"):
            _capi.bcs_gram(**kw)
    for bad in (dict(sigma2=-1.0), dict(sigma2=np.inf), dict(scale=0.0), dict(scale=-1.0), dict(scale=np.nan), dict(eta=-1e-3),
                dict(eta=np.nan), dict(itermax=0), dict(max_active=5), dict(max_active=-1)):
        with pytest.raises(ValueError, match="fsnap_bcs_gram"):
            _capi.bcs_gram(Q, q, y2, sy, n, **bad)
    with pytest.raises(ValueError):
        _capi.bcs_gram(Q, q, y2, sy, n, deletion="textbook")
    with pytest.raises(ValueError):
        _capi.bcs_gram(Q[:3], q, y2, sy, n)
    # the raw entry point: NULL pointers, K < 1, an unknown deletion code
    lib = _capi.load_library()
    out = [np.zeros(16) for _ in range(5)]
    io = [np.zeros(32, dtype=np.int32) for _ in range(2)]

    def status(K=4, Qp=Q, qp=q, deletion=0, coef=out[0], active=io[0], alpha=out[1], mu=out[2], err=out[3], Sig=out[4],
               picks=io[1], info=np.zeros(6)):
        return lib.fsnap_bcs_gram(K, _capi._ptr(Qp), _capi._ptr(qp), y2, sy, n, None, 0.0, 0.01, ETA, 10, min(max(K, 1), 4), deletion,
                                  *(_capi._ptr(x) for x in (coef, active, alpha, mu, err, Sig, picks, info)))

    assert status() == _capi.OK
    for bad in (dict(K=0), dict(Qp=None), dict(qp=None), dict(deletion=2), dict(deletion=-1), dict(coef=None), dict(active=None),
                dict(alpha=None), dict(mu=None), dict(err=None), dict(Sig=None), dict(picks=None), dict(info=None)):
        assert status(**bad) == _capi.E_ARG, bad


def test_bcs_config_section():
    sec = Config(None, {"SOLVER": {"solver": "BCS"}}).sections["BCS"]
    assert (sec.sigma2, sec.scale, sec.eta, sec.itermax, sec.max_active, sec.deletion) == (None, 0.01, 1e-18, 10, 0, "reference")
    sec = Config(None, {"SOLVER": {"solver": "BCS"}, "BCS": {"sigma2": "2.5e-3", "Scale": "0.1", "eta": "1e-8", "itermax": "80",
                                                           "max_active": "12", "deletion": "Exact"}}).sections["BCS"]
    assert (sec.sigma2, sec.scale, sec.eta, sec.itermax, sec.max_active, sec.deletion) == (2.5e-3, 0.1, 1e-8, 80, 12, "exact")
    assert Config(None, {"SOLVER": {"solver": "bcs"}, "BCS": {"sigma2": ""}}).sections["BCS"].sigma2 is None
    with pytest.raises(RuntimeError, match="unmatched variable in BCS"):
        Config(None, {"SOLVER": {"solver": "BCS"}, "BCS": {"sigma": 3}})
    with pytest.raises(UserWarning, match="BCS section is in input"):
        Config(None, {"SOLVER": {"solver": "RIDGE"}, "BCS": {"itermax": 3}})
    for bad in ({"sigma2": "0"}, {"sigma2": "-1"}, {"sigma2": "small"}, {"scale": "0"}, {"eta": "-1"}, {"itermax": "0"},
                {"max_active": "-2"}, {"deletion": "textbook"}):
        with pytest.raises(RuntimeError):
            Config(None, {"SOLVER": {"solver": "BCS"}, "BCS": bad})
    assert "BCS" not in Config(None, {"SOLVER": {"solver": "RIDGE"}}).sections


def bcs_on_statistics(monkeypatch, stats, section=None, extra=None):
    """A BCS solver from the factory whose statistics pass is replaced by ``stats`` (G, c, (bb, sum wb, n)): the rest of
    ``perform_fit`` is host algebra."""
    pt = ParallelTools()
    d = {"SOLVER": {"solver": "BCS"}, "BCS": dict(section or {})}
    d.update(extra or {})
    s = solver_factory.solver("BCS", pt, Config(pt, d))
    assert type(s).__name__ == "BCS"
    monkeypatch.setattr(s, "_fit_statistics", lambda *a, **k: stats)
    return s


@pytest.mark.parametrize("tag", ["ta", "ta_testing", "ta_transpose"])
def test_solver_through_the_factory(ta, tag, monkeypatch):
    want = cs.expected(tag)
    A, b, w = ta
    keep = ~cs.golden()[f"{tag}_testing"]
    Q, q, y2, sy, n = cs.statistics_ld((w[:, None] * A)[keep], (w * b)[keep])
    extra = {"SOLVER": {"solver": "BCS", "nsam": 7}}
    if tag == "ta_transpose":
        extra["EXTRAS"] = {"apply_transpose": 1}
    s = bcs_on_statistics(monkeypatch, (Q, q, np.array([y2, sy, n])), extra=extra)
    np.random.seed(11)
    s.perform_fit()
    K = A.shape[1]
    fit = np.zeros(K)
    fit[want["used"]] = want["weights"]
    cov = np.diag(fit ** 2)
    cov[np.ix_(want["used"], want["used"])] = want["Sig"]
    assert s.used.tolist() == want["used"].tolist()
    assert cs.rel(s.fit, fit) < cs.REF_BAR and cs.rel(s.errbars, want["errbars"]) < cs.REF_BAR
    assert abs(s.sigma2 - float(want["sigma2"])) < cs.REF_BAR * float(want["sigma2"])
    off = np.ones((K, K), dtype=bool)
    off[np.ix_(want["used"], want["used"])] = False
    assert cs.rel(s.cov, cov) < cs.REF_BAR and not s.cov[off].any() and s.cov.min() >= 0.0
    # fit_sam: drawn as the reference draws it, from numpy's global generator
    np.random.seed(11)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sam = np.random.multivariate_normal(s.fit, s.cov, size=(7,))
    assert s.fit_sam.shape == (7, K) and np.array_equal(s.fit_sam, sam)
    s.pt.free()


def test_solver_without_samples_and_a_refused_max_active(ta, monkeypatch):
    A, b, w = ta
    Q, q, y2, sy, n = cs.statistics_ld(w[:, None] * A, w * b)
    s = bcs_on_statistics(monkeypatch, (Q, q, np.array([y2, sy, n])), {"itermax": 40, "deletion": "exact", "scale": 1e-4})
    s.perform_fit()
    assert getattr(s, "fit_sam", None) is None and np.count_nonzero(s.fit) == s.used.size > 8
    assert s.bcs.iterations <= 40 and s.errbars.shape == s.used.shape
    s.pt.free()
    s = bcs_on_statistics(monkeypatch, (Q, q, np.array([y2, sy, n])), {"max_active": 99})
    with pytest.raises(ValueError, match="max_active"):
        s.perform_fit()
    s.pt.free()


def test_grid_and_route_checks():
    sec = Config(None, {"SOLVER": {"solver": "BCS"}, "BCS": {"itermax": 20}}).sections["BCS"]
    grid = bp.resolve_grid([0.1, {"sigma2": 2.0, "eta": 1e-6}, {"itermax": 5.0}], sec)
    assert grid == [{"scale": 0.1, "sigma2": None, "eta": 1e-18, "itermax": 20}, {"scale": 0.01, "sigma2": 2.0, "eta": 1e-6, "itermax": 20},
                    {"scale": 0.01, "sigma2": None, "eta": 1e-18, "itermax": 5}]
    assert bp.hyper_of(grid).tolist() == [[0.0, 0.1, 1e-18, 20.0], [2.0, 0.01, 1e-6, 20.0], [0.0, 0.01, 1e-18, 5.0]]
    for bad in ([], {"scale": 1.0}, "0.1", 3.0, [{"alpha": 1.0}], [{"scale": 0.0}], [{"scale": np.nan}], [{"sigma2": -1.0}],
                [{"eta": -1.0}], [{"itermax": 0}], [{"itermax": 2.5}], [{"itermax": 65537}], [{"max_active": 3}]):
        with pytest.raises(ValueError):
            bp.resolve_grid(bad, sec)
    assert bp.resolve_max_active(0, 200) == 64 and bp.resolve_max_active(0, 7) == 7 and bp.resolve_max_active(3, 7) == 3
    with pytest.raises(ValueError):
        bp.resolve_max_active(8, 7)
    assert bp.choose_method("auto", 144, 64) == "device" and bp.choose_method("auto", 145, 64) == "host"
    assert bp.choose_method("auto", 200, 100) == "host" and bp.choose_method("host", 10, 5) == "host"
    for bad in (("device", 145, 64), ("device", 144, 65), ("gpu", 10, 10)):
        with pytest.raises(ValueError):
            bp.choose_method(*bad)
    pt = ParallelTools()
    for name, extra, match in (("RIDGE", {}, "has no BCS path"), ("ARD", {}, "has no BCS path"),
                               ("BCS", {"EXTRAS": {"apply_transpose": 1}}, "apply_transpose")):
        sol = solver_factory.solver(name, pt, Config(pt, {"SOLVER": {"solver": name}, **extra}))
        with pytest.raises(ValueError, match=match):
            sol.bcs_path([0.01])
    sol = solver_factory.solver("BCS", pt, Config(pt, {"SOLVER": {"solver": "BCS"}}))
    with pytest.raises(ValueError, match="empty"):
        sol.bcs_path([])
    with pytest.raises(ValueError, match="unknown grid key"):
        sol.bcs_path([{"logcut": 1.0}])
    pt.free()


@pytest.mark.parametrize("name", ["k2", "k63", "loco"])
def test_host_route_on_blocks(name):
    """``bcs_path_host`` on hand-made blocks: every problem is ``bcs_gram`` on the downdated system with the problem's own
    sigma2, the held-out record is the statistics form, and the picks follow ``ard_path.cv_picks``."""
    blocks, K, F, nsub, hyper, ma, deletion = cs.case_blocks(name)
    coef, active, alpha, err, picks, info, held, Sig = cs.case_host(name)
    Q = hyper.shape[0]
    assert coef.shape == (F + 1, Q, K) and active.shape == (F + 1, Q, ma) and picks.shape == (F + 1, Q, int(hyper[:, 3].max()), 2)
    assert held.shape == (F, Q, 3) and Sig.shape == (Q, ma, ma)
    folds, total = ff.sum_blocks(blocks, nsub)
    for f in sorted({0, F - 1, F}):
        Qm, qv, y2, sum_y, n, tdiag = cs.downdated_scalars(blocks, nsub, f, K)
        for q in range(Q):
            s2, scale, eta, it = hyper[q]
            r = _capi.bcs_gram(Qm, qv, y2, sum_y, n, s2 if s2 > 0 else None, scale, eta, int(it), ma, deletion, tdiag)
            na = r.active.size
            assert np.array_equal(coef[f, q], r.coef) and active[f, q, :na].tolist() == r.active.tolist()
            assert np.all(active[f, q, na:] == -1) and np.array_equal(err[f, q, :na], r.errbars)
            assert np.array_equal(picks[f, q, :int(it)], r.picks) and np.all(picks[f, q, int(it):] == -1)
            assert info[f, q].tolist() == [r.iterations, r.status, r.sigma2_in, r.sigma2, r.rss, r.margin]
            if s2 == 0:
                assert r.sigma2_in == max(scale * (y2 / n - (sum_y / n) ** 2), 1e-16)
            if f < F:
                G, c, bb, nf = ff.unpack(folds[f], K)
                assert held[f, q].tolist() == [nf, bb - 2.0 * (r.coef @ c) + r.coef @ (G @ r.coef), bb]
            else:
                assert np.array_equal(Sig[q, :na, :na], r.Sig) and not Sig[q, na:].any()
    status = info[:, :, 1].astype(np.int64)
    nonzeros = np.count_nonzero(coef[F], axis=1)
    cv_error, cv_se, best, sparsest = ap.cv_picks(held, status, nonzeros)
    assert np.all(np.isfinite(cv_error)) and best == int(np.argmin(cv_error))
    assert nonzeros[sparsest] <= nonzeros[best] and cv_error[sparsest] <= cv_error[best] + cv_se[best]
    np.testing.assert_allclose(cv_error, held[:, :, 1].sum(axis=0) / held[:, :, 0].sum(axis=0), rtol=1e-14)
    freq = bp.keep_frequency(active[:F], best, K)
    assert 0.0 <= freq.min() and freq.max() <= 1.0 and freq.sum() * F == (active[:F, best] >= 0).sum()
    covs = bp.covariances(coef[F], active[F], Sig)
    for q in range(Q):
        sup = active[F, q][active[F, q] >= 0]
        assert np.array_equal(np.diag(covs[q])[sup], np.maximum(np.diag(Sig[q])[:sup.size], 0.0)) and covs[q].min() >= 0.0


def test_host_route_dead_column_and_an_empty_training_set():
    blocks, K = cs.edge_blocks(3)
    hyper = bp.hyper_of(bp.resolve_grid([0.01], type("S", (), dict(sigma2=None, scale=0.01, eta=1e-18, itermax=12))))
    coef, active, _, _, picks, info, held, _ = bp.bcs_path_host(blocks, K, hyper, K, "reference")
    assert np.all(coef[:, 0, 3] == 0.0) and not (active == 3).any()          # the zero column is dead everywhere
    assert coef[1, 0, 7] == 0.0 and not (active[1] == 7).any()               # fold 1 alone touches column 7
    assert all(coef[f, 0, 7] != 0.0 for f in (0, 2, 3))
    # one fold holds every row: its refit has no training rows, no live column, and predicts zero
    coef, active, _, _, picks, info, held, _ = bp.bcs_path_host(blocks.sum(axis=0, keepdims=True), K, hyper, K, "reference")
    assert not coef[0].any() and np.all(active[0] == -1) and info[0, 0, 0] == 0 and info[0, 0, 1] == 0
    assert held[0, 0, 1] == held[0, 0, 2] and np.count_nonzero(coef[1]) > 0
