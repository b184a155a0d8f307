"""The ranking step of a Bayesian active-learning loop on the golden Ta rows, on the GPU
(Solver.prediction_variance; the reference's examples/library/bayesian_active_learning/bayesian_active_learning.py ranks
the unlabeled pool by the predictive variance diag = (A C * A).sum(-1) of a fresh ANL fit on every iteration).

The fixture has no configuration labels, so the unit of selection is the GROUP (ea_groups of ta_reference_fits.npz): some
groups are held out as the pool, ANL is fitted on the rest, the pool groups are ranked by their summed scaled variance
(row scale w^2, the fit's own energy / force / stress weighting), the top one moves into the training set, and the fit is
repeated.  The *ALL error rows of every iteration are printed.

    python examples/active_learning_uncertainty.py [--iterations N] [--check]

--check compares the first ranking with the numpy expression (A @ C * A).sum(-1) summed per group.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from fitsnap_amd.config import Config  # noqa: E402
from fitsnap_amd.parallel_tools import ParallelTools  # noqa: E402
from fitsnap_amd.solvers import solver_factory  # noqa: E402

ROW_TYPE = ["Energy"] * 363 + ["Force"] * 12672 + ["Stress"] * 2178


def main(iterations=4, check=False):
    z = np.load(os.path.join(ROOT, "tests", "golden", "ta_abw.npz"))
    f = np.load(os.path.join(ROOT, "tests", "golden", "ta_reference_fits.npz"))
    A, b, w = (np.ascontiguousarray(z[k]) for k in ("A", "b", "w"))
    groups = np.array([str(g) for g in f["ea_groups"]])
    names = sorted(set(groups))
    rng = np.random.default_rng(0)
    pool = set(rng.choice(names, len(names) // 2, replace=False).tolist())
    pt = ParallelTools()
    s = solver_factory.solver("ANL", pt, Config(pt, {"SOLVER": {"solver": "ANL"}}))
    s.save_files = False
    for it in range(iterations):
        in_pool = np.isin(groups, sorted(pool))
        tr = ~in_pool
        s.perform_fit(np.ascontiguousarray(A[tr]), np.ascontiguousarray(b[tr]), w[tr], trainall=True)
        Ap = np.ascontiguousarray(A[in_pool])
        pool_groups = groups[in_pool].tolist()
        res = s.prediction_variance(Ap, categories=pool_groups, row_scale=w[in_pool] ** 2, method="fullcov")
        order = np.argsort(-res["cat_sum"], kind="stable")
        ranking = [res["keys"][i] for i in order]
        if check and it == 0:
            diag = (Ap @ s.cov * Ap).sum(-1) * w[in_pool] ** 2
            ref = {g: 0.0 for g in res["keys"]}
            for g, v in zip(pool_groups, diag):
                ref[g] += v
            ref_rank = sorted(ref, key=lambda g: -ref[g])
            assert ranking == ref_rank, (ranking, ref_rank)
            assert np.allclose(res["cat_sum"], [ref[g] for g in res["keys"]], rtol=1e-10, atol=0)
            print("first ranking matches numpy (A @ C * A).sum(-1) summed per group")
        fs = {"Groups": groups.tolist(), "Testing": in_pool.tolist(), "Row_Type": ROW_TYPE}
        s.error_analysis(A, b, w, fs)
        allrows = s.errors.loc["*ALL"]
        print(f"iteration {it}: {tr.sum()} training rows, {len(pool)} pool groups, top {ranking[:3]}")
        for idx, row in allrows.iterrows():
            print(f"  *ALL {idx}: " + ", ".join(f"{k} {v:.4g}" for k, v in row.items()))
        pool.discard(ranking[0])
        if not pool:
            break
    pt.free()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=4)
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    main(args.iterations, args.check)
