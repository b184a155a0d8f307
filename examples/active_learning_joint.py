"""Joint selection criteria for a Bayesian active-learning batch on the golden Ta rows, on the GPU
(Solver.unit_scores / Solver.select_units next to Solver.select_batch).

``select_batch`` scores a configuration by the sum (max, mean) of its rows' MARGINAL variances.  The rows of a configuration
are strongly correlated, so the sum counts the same information many times and favours large cells, and a configuration of
high own variance may be an outlier that says little about the rest of the pool.  For a linear model both have exact,
label-free cures, one small Cholesky factor per configuration:

    gain       1/2 logdet(I + X C X^T / noise): the information the configuration's labels carry, all rows at once
    reduction  tr(T C) - tr(T C'): how much the total predictive variance over a TARGET set drops (here the pool itself,
               rows scaled by w^2) -- the integrated-variance criterion

The fixture has no configuration labels: the rows are cut into synthetic configurations of 1 ... 120 consecutive rows.  A
random quarter of them is the pool, ANL is fitted on the rest.  Three greedy batches are selected -- by gain, by pool-targeted
reduction, by select_batch("sum") -- and for each the information gained (1/2 logdet of the batch as a whole) and the total
pool variance it leaves are printed.

    python examples/active_learning_joint.py [--batch B] [--check]

--check compares the two joint selections with the numpy statement of the loop (select_joint.greedy_joint_host).
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from fitsnap_amd.config import Config  # noqa: E402
from fitsnap_amd.parallel_tools import ParallelTools  # noqa: E402
from fitsnap_amd.solvers import select, select_joint, solver_factory  # noqa: E402


def configurations(m, seed=5, lo=1, hi=120):
    rng = np.random.default_rng(seed)
    sizes = []
    while sum(sizes) < m:
        sizes.append(int(rng.integers(lo, hi + 1)))
    sizes[-1] -= sum(sizes) - m
    return np.repeat(np.arange(len(sizes)), sizes)


def batch_outcome(keys, cfg, Ap, wp, C0, noise, scale):
    """(information gained by the batch as a whole, total pool variance left) of a batch of configurations."""
    rows = np.flatnonzero(np.isin(cfg, [int(k[3:]) for k in keys]))
    X = wp[rows, None] * Ap[rows]
    info = select_joint.score_one(X, select_joint.factor_cov(C0), noise)[0]
    C = select.downdate_cov(C0, select.downdate_factor(C0, X, noise))
    return info, float((((Ap @ C) * Ap).sum(-1) * scale).sum())


def main(batch=8, check=False):
    z = np.load(os.path.join(ROOT, "tests", "golden", "ta_abw.npz"))
    A, b, w = (np.ascontiguousarray(z[k]) for k in ("A", "b", "w"))
    cfg_all = configurations(len(b))
    ncfg = int(cfg_all.max()) + 1
    pool_cfg = np.sort(np.random.default_rng(0).choice(ncfg, ncfg // 4, replace=False))
    in_pool = np.isin(cfg_all, pool_cfg)
    pt = ParallelTools()
    s = solver_factory.solver("ANL", pt, Config(pt, {"SOLVER": {"solver": "ANL"}}))
    s.save_files = False
    s.perform_fit(np.ascontiguousarray(A[~in_pool]), np.ascontiguousarray(b[~in_pool]), w[~in_pool], trainall=True)
    Ap, wp = np.ascontiguousarray(A[in_pool]), np.ascontiguousarray(w[in_pool])
    cfg = cfg_all[in_pool]
    scale = wp ** 2
    labels = [f"cfg{c}" for c in cfg]
    one = s.unit_scores(a=Ap, w=wp, categories=labels, row_scale=scale)
    print(f"{len(Ap)} pool rows in {len(one['keys'])} configurations, noise variance {s.sigmahat:.4g}, "
          f"total pool variance {one['total']:.6g}")
    gain = s.select_units(batch, a=Ap, w=wp, categories=labels, criterion="gain")
    red = s.select_units(batch, a=Ap, w=wp, categories=labels, criterion="reduction", row_scale=scale)
    marg = s.select_batch(batch, a=Ap, w=wp, categories=labels, row_scale=scale, objective="sum")
    for name, keys in (("gain", gain.keys), ("reduction", red.keys), ("select_batch sum", marg.keys)):
        info, left = batch_outcome(keys, cfg, Ap, wp, s.cov, s.sigmahat, scale)
        nrows = int(np.isin(cfg, [int(k[3:]) for k in keys]).sum())
        print(f"{name:>17}: {' '.join(keys)}")
        print(f"{'':>17}  {nrows} rows, information gained {info:.4f} nats, pool variance left {left:.6g}")
    if check:
        T = Ap.T @ (scale[:, None] * Ap)
        for res, crit in ((gain, "gain"), (red, "reduction")):
            host = select_joint.greedy_joint_host(Ap, cfg, ncfg, s.cov, wp, s.sigmahat, batch, crit, T)
            assert [f"cfg{c}" for c in host["picks"]] == res.keys, (crit, host["picks"], res.keys)
            # the two runs differ in the rounding of the target Gram (statistics kernel against numpy) and of the scores; the
            # information matrix of this fit has condition 7e10, which that rounding passes through: kappa eps = 1.5e-5
            assert np.allclose(res.scores, host["scores"], rtol=1e-6, atol=0), (crit, res.scores, host["scores"])
            assert np.allclose(res.cov, host["cov"], rtol=0, atol=1e-12 * np.abs(host["cov"]).max())
        print("joint selections match the numpy statement (select_joint.greedy_joint_host)")
    pt.free()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    main(args.batch, args.check)
