"""Choosing the singular-value cut and the ridge penalty of a linear fit by grouped cross-validation, on the GPU
(Solver.spectral_path).

An SVD fit has one knob, the cut rcond of lstsq(aw, bw, rcond), and a RIDGE fit one, the penalty alpha.  One SVD fit of the
synthetic workload, then ONE pass over the rows for the statistics of every (fold, row type) and ONE symmetric eigendecomposition
per fold of "total minus fold": every (alpha, rcond) of the grid is then a filter on the eigenpairs.  Printed: rank, effective
number of parameters, training and generalised cross-validation error, the held-out error with its standard error over the
folds, the best setting and the simplest one within one standard error of it, and the spectrum of the fit on all rows.

    python examples/spectral_path.py [--rows M] [--columns K] [--folds F] [--method auto|device|host] [--table auto|rows|stats]
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
from fitsnap_amd.synthetic import synth_problem  # noqa: E402

RCONDS = [1e-13, 1e-8, 1e-6, 1e-4]


def main(m=20000, K=64, folds=5, method="auto", table="stats"):
    A, b, w = synth_problem(m, K)
    pt = ParallelTools()
    s = solver_factory.solver("SVD", pt, Config(pt, {"SOLVER": {"solver": "SVD"}}))
    for name, arr in (("a", A), ("b", b), ("w", w)):
        pt.create_shared_array(name, m, K if name == "a" else 1)
        pt.shared_arrays[name].array[:] = arr
    pt.fitsnap_dict.update({"Configs": [f"c{i // 25}" for i in range(m)], "Testing": [False] * m,
                            "Row_Type": [("Energy", "Force", "Stress")[i % 3] for i in range(m)]})
    s.perform_fit()
    lam_max = float(np.linalg.eigvalsh(s.last_statistics[0])[-1])
    alphas = [0.0] + [x * lam_max for x in (1e-12, 1e-9, 1e-6, 1e-3)]
    res = s.spectral_path(alphas, RCONDS, folds=folds, method=method, table=table)
    F = len(set(res.fold_of_unit.values()))
    print(f"{F}-fold cross-validation (by Configs) of {len(alphas)} alphas x {len(RCONDS)} rconds on {m} x {K} synthetic rows; "
          f"Jacobi sweeps per problem {res.sweeps.tolist()}")
    print(f"{'alpha':>10} {'rcond':>8} {'rank':>5} {'dof':>8} {'train sse':>12} {'gcv':>12} {'cv error':>12} {'+- se':>10} {'w_rmse':>12}")
    for q, (a, r) in enumerate(res.grid):
        mark = " <- best" if q == res.best else (" <- simplest within one se" if q == res.simplest else "")
        print(f"{a:10.3e} {r:8.1e} {int(res.rank[F, q]):5d} {res.dof[F, q]:8.3f} {res.train_sse[F, q]:12.6g} {res.gcv[q]:12.6g} "
              f"{res.cv_error[q]:12.6g} {res.cv_se[q]:10.3g} {res.table.loc[(a, r, '*ALL'), 'w_rmse']:12.6g}{mark}")
    print(f"best: alpha = {res.best_alpha:.3e}, rcond = {res.best_rcond:.1e}; simplest within one standard error: alpha = "
          f"{res.simplest_alpha:.3e}, rcond = {res.simplest_rcond:.1e}")
    print(res.table.loc[(res.best_alpha, res.best_rcond)].to_string())
    lam = res.eigenvalues[F]
    print(f"spectrum of the fit on all rows: lambda_max = {lam.max():.3e}, lambda_min = {lam[lam != 0].min():.3e}, "
          f"condition number {lam.max() / lam[lam != 0].min():.3e}")
    pt.free()


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--rows", type=int, default=20000)
    ap.add_argument("--columns", type=int, default=64)
    ap.add_argument("--folds", type=int, default=5)
    ap.add_argument("--method", default="auto", choices=["auto", "device", "host"])
    ap.add_argument("--table", default="stats", choices=["auto", "rows", "stats"])
    a = ap.parse_args()
    main(a.rows, a.columns, a.folds, a.method, a.table)
