"""The batch step of a Bayesian active-learning loop on the golden Ta rows, on the GPU (Solver.select_batch).

The reference's loop (examples/library/bayesian_active_learning/bayesian_active_learning.py:887-909) takes ``batch_size``
structures per iteration from ONE ranking of the pool by predictive variance; near-copies of a structure rank next to
each other, so it clusters the pool with k-means to spread the batch.  For a linear model the posterior after adding a
structure is known before its labels are, so every pick can be made against the posterior that already contains the
earlier picks: greedy variance reduction, exact, without refits.

The fixture has no configuration labels: the rows are cut into synthetic configurations of 1 ... 120 consecutive rows.  A
random quarter of the configurations is the pool, ANL is fitted on the rest; a batch is selected greedily and, for
comparison, as the top B of the one-shot ranking (row scale w^2, the fit's own energy / force / stress weighting).  Both
batches and the total pool variance each leaves (sum of w_i^2 a_i^T C a_i over the pool rows under the posterior that
contains the batch) are printed.  The training rows cover this pool well, so the two batches mostly coincide here; they
part where the pool holds redundant configurations that the training set does not cover (tests/select_cases.py).

    python examples/active_learning_batch.py [--batch B] [--objective sum|max|mean] [--check]

--check compares the greedy batch with the numpy statement of the loop (fitsnap_amd.solvers.select.greedy_host).
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from fitsnap_amd.config import Config  # noqa: E402
from fitsnap_amd.parallel_tools import ParallelTools  # noqa: E402
from fitsnap_amd.solvers import select, solver_factory  # noqa: E402


def configurations(m, seed=5, lo=1, hi=120):
    rng = np.random.default_rng(seed)
    sizes = []
    while sum(sizes) < m:
        sizes.append(int(rng.integers(lo, hi + 1)))
    sizes[-1] -= sum(sizes) - m
    return np.repeat(np.arange(len(sizes)), sizes)


def pool_variance(Ap, C, scale):
    return float((((Ap @ C) * Ap).sum(-1) * scale).sum())


def main(batch=8, objective="sum", check=False):
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
    res = s.select_batch(batch, a=Ap, w=wp, categories=labels, row_scale=scale, objective=objective)
    print(f"{len(Ap)} pool rows in {len(res.all_keys)} configurations, noise variance {s.sigmahat:.4g}, objective {objective}")
    print(f"total pool variance before: {pool_variance(Ap, s.cov, scale):.6g}")
    print("greedy batch: " + " ".join(f"{k}({j})" for k, j in zip(res.keys, res.ranks)))
    print(f"  total pool variance left: {pool_variance(Ap, res.cov, scale):.6g}")
    # the top B of the one ranking, and the posterior that contains them
    order = np.argsort(-np.where(np.isnan(res.initial_scores), -np.inf, res.initial_scores), kind="stable")[:batch]
    top = [res.all_keys[i] for i in order]
    C = s.cov
    for key in top:
        rows = np.flatnonzero(cfg == int(key[3:]))
        C = select.downdate_cov(C, select.downdate_factor(C, wp[rows, None] * Ap[rows], s.sigmahat))
    print("top-B batch:  " + " ".join(top))
    print(f"  total pool variance left: {pool_variance(Ap, C, scale):.6g}")
    print(f"{len(set(top) - set(res.keys))} of the {batch} picks differ")
    if check:
        host = select.greedy_host(Ap, cfg, ncfg, s.cov, wp, s.sigmahat, batch, scale, objective)
        assert [f"cfg{c}" for c in host["picks"]] == res.keys, (host["picks"], res.keys)
        # scores: sums of rows whose two evaluations differ by the rounding of a^T C a and of the ||a V||^2 taken off it
        eps, aa, K = np.finfo(np.float64).eps, np.abs(Ap), Ap.shape[1]
        bar = 4 * K * eps * ((aa @ np.abs(s.cov)) * aa).sum(-1)
        for V in host["factors"]:
            bar += 4 * (K + V.shape[1]) * eps * ((aa @ np.abs(V)) ** 2).sum(-1)
        for u, got, want in zip(host["picks"], res.scores, host["scores"]):
            assert abs(got - want) <= (scale * bar)[cfg == u].sum() + 256 * eps * abs(want), (u, got, want)
        assert np.allclose(res.cov, host["cov"], rtol=0, atol=1e-12 * np.abs(host["cov"]).max())
        print("greedy batch matches the numpy statement (select.greedy_host)")
    pt.free()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--objective", default="sum")
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    main(args.batch, args.objective, args.check)
