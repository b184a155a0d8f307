"""CPU: the MERR solver is registered and configured like the reference's, and the host's gradient composition
(fitsnap_amd/solvers/merr.py) is the gradient of the log-posterior (lreg.py logpost_emb, restated here in numpy)."""
import numpy as np
import pytest

from fitsnap_amd import _capi
from fitsnap_amd.config import Config
from fitsnap_amd.parallel_tools import ParallelTools
from fitsnap_amd.solvers import solver_factory
from fitsnap_amd.solvers.merr import MERR, embedded_columns, merr_constant, merr_gradient, merr_q


def logpost(x, aw, bw, ind, datavar, mult, method):
    """numpy restatement of the reference's logpost_emb (diagonal 'full' is 'iid')."""
    nbas = aw.shape[1]
    cf, sig = x[:nbas], x[nbas:]
    if mult:
        sig = np.abs(cf[ind]) * sig
    ss = aw[:, ind] * sig
    err = aw @ cf - bw
    stds = np.sqrt(np.sum(ss * ss, axis=1) + datavar)
    if method == "abc":
        r = np.abs(err) - stds
        return -0.5 * np.sum((r / 0.1) ** 2) - 0.5 * np.log(2 * np.pi) - np.log(0.1)
    return -0.5 * np.sum((err / stds) ** 2) - 0.5 * len(bw) * np.log(2 * np.pi) - np.sum(np.log(stds))


def host_sums(aw, bw, cf, q, d, method):
    """(val, g, h) of one pass, computed here in numpy (what fsnap_merr_eval returns)."""
    e = aw @ cf - bw
    v = (aw * aw) @ q + d
    if method == "abc":
        sv = np.sqrt(v)
        r = np.abs(e) - sv
        val, al, be = np.sum(-0.5 * r * r / 0.01), -r / 0.01 * np.sign(e), r / (0.02 * sv)
    else:
        val, al, be = np.sum(-0.5 * e * e / v - 0.5 * np.log(v)), -e / v, 0.5 * e * e / v ** 2 - 0.5 / v
    return val, aw.T @ al, (aw * aw).T @ be


def test_search_finds_merr():
    assert type(solver_factory.search("MERR")) is MERR
    assert type(solver_factory.search("merr")) is MERR


def test_config_merr_defaults_and_values():
    cfg = Config(None, {"SOLVER": {"solver": "MERR"}})
    sec = cfg.sections["SOLVER"]
    assert sec.merr_mult is False and sec.merr_method == "abc" and sec.merr_cfs == "all"
    cfg = Config(None, {"SOLVER": {"solver": "MERR", "merr_mult": "1", "merr_method": "iid", "merr_cfs": "0 2 5"}})
    sec = cfg.sections["SOLVER"]
    assert sec.merr_mult is True and sec.merr_method == "iid" and sec.merr_cfs == "0 2 5"


@pytest.mark.parametrize("method", ["iid", "abc"])
@pytest.mark.parametrize("mult", [False, True])
@pytest.mark.parametrize("ind", [None, [0, 2, 5]])
def test_gradient_composition_matches_central_differences(method, mult, ind):
    r = np.random.default_rng(4)
    n, K = 400, 6
    aw = r.standard_normal((n, K))
    bw = aw @ r.standard_normal(K) + 0.2 * r.standard_normal(n)
    emb = np.arange(K) if ind is None else np.array(ind)
    d = 0.05
    x = np.concatenate([r.standard_normal(K), 0.2 + r.random(len(emb))])
    cf, sig = x[:K], x[K:]
    val, g, h = host_sums(aw, bw, cf, merr_q(cf, sig, emb, mult), d, method)
    L = val + merr_constant(method, n)
    assert abs(L - logpost(x, aw, bw, emb, d, mult, method)) <= 1e-10 * abs(L)
    gc, gs = merr_gradient(cf, sig, emb, mult, g, h)
    grad = np.concatenate([gc, gs])
    for k in range(len(x)):
        hk = 1e-6 * max(1.0, abs(x[k]))
        xp, xm = x.copy(), x.copy()
        xp[k] += hk
        xm[k] -= hk
        fd = (logpost(xp, aw, bw, emb, d, mult, method) - logpost(xm, aw, bw, emb, d, mult, method)) / (2 * hk)
        assert abs(fd - grad[k]) <= 1e-6 * max(1.0, np.max(np.abs(grad))), (k, fd, grad[k])


def test_merr_cfs_maps_reduced_columns_past_dropped_zero_columns():
    keep = np.array([True, True, False, True, False, True, True])
    cols = np.flatnonzero(keep)                      # reduced column i is full column cols[i]
    emb = embedded_columns("0 2 4", len(cols))
    assert list(cols[emb]) == [0, 3, 6]
    assert list(embedded_columns("all", 5)) == [0, 1, 2, 3, 4]
    with pytest.raises(AssertionError):
        embedded_columns("6", 5)                     # merr.py: assert int(i) <= nbas


def test_merr_perform_fit_without_gpu_raises():
    if _capi.device_count() > 0:
        pytest.skip("a GPU is present")
    pt = ParallelTools()
    cfg = Config(pt, {"SOLVER": {"solver": "MERR"}})
    s = solver_factory.solver("MERR", pt, cfg)
    r = np.random.default_rng(0)
    with pytest.raises(Exception):
        s.perform_fit(r.standard_normal((50, 4)), r.standard_normal(50), np.ones(50), trainall=True)
    assert s.fit is None
