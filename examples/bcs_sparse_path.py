"""Choosing the sparsity of a BCS fit by grouped cross-validation on the golden Ta rows, on the GPU (Solver.bcs_path).

The initial noise variance of Bayesian compressive sensing sets how many descriptors the fit keeps, and the iteration cap how
far the recurrence gets; the reference fixes both.  One BCS fit, then ONE pass over the rows for the statistics of every fold
and, for every setting of a grid, the BCS refit without each fold on "total minus fold": the held-out error per setting with
its standard error over the folds, the number of descriptors kept, the setting with the smallest error, the sparsest setting
within one standard error of it, how often every descriptor was kept, and the error bars that come with the chosen fit.

    python examples/bcs_sparse_path.py [--by Groups|Configs] [--folds F] [--method auto|device|host] [--deletion reference|exact]

The fixture has no configuration labels; --by Configs takes blocks of 7 consecutive rows as stand-ins and deals them into
--folds folds.
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
GRID = [{"scale": s, "itermax": 80, "eta": 1e-8} for s in (1e-1, 1e-2, 1e-3, 1e-4, 1e-5, 1e-6)] + [{"scale": 1e-2, "itermax": 10}]


def main(by="Configs", folds=5, method="auto", deletion="reference"):
    z = np.load(os.path.join(ROOT, "tests", "golden", "ta_abw.npz"))
    f = np.load(os.path.join(ROOT, "tests", "golden", "ta_reference_fits.npz"))
    A, b, w = (np.ascontiguousarray(z[k]) for k in ("A", "b", "w"))
    m, K = A.shape
    pt = ParallelTools()
    s = solver_factory.solver("BCS", pt, Config(pt, {"SOLVER": {"solver": "BCS"}, "BCS": {"deletion": deletion}}))
    for name, arr in (("a", A), ("b", b), ("w", w)):
        pt.create_shared_array(name, m, K if name == "a" else 1)
        pt.shared_arrays[name].array[:] = arr
    pt.fitsnap_dict.update({"Groups": [str(g) for g in f["ea_groups"]], "Testing": [False] * m, "Row_Type": ROW_TYPE,
                            "Configs": [f"c{i // 7}" for i in range(m)]})
    s.perform_fit()
    print(f"BCS as the reference runs it (scale 0.01, 10 iterations): {s.used.size} of {K} descriptors, sigma2 {s.sigma2:.4g}")
    res = s.bcs_path(GRID, folds=None if by == "Groups" else folds, by=by, method=method)
    nfolds = len(set(res.fold_of_unit.values()))
    print(f"{nfolds}-fold cross-validation (by {by}) of the BCS fit on {m} x {K} Ta rows, {len(GRID)} settings, deletion = {deletion}")
    print(f"{'scale':>8} {'itermax':>7} {'kept':>5} {'iter':>5} {'cv error':>12} {'+- se':>10} {'mae':>12} {'rmse':>12} {'w_rmse':>12}")
    for q, g in enumerate(res.grid):
        r = res.table.loc[(q, "*ALL")]
        mark = " <- best" if q == res.best else (" <- sparsest within one se" if q == res.sparsest else "")
        print(f"{g['scale']:8.1e} {g['itermax']:7d} {int(res.nonzeros[q]):5d} {int(res.iterations[-1, q]):5d} "
              f"{res.cv_error[q]:12.6g} {res.cv_se[q]:10.3g} {r['mae']:12.6g} {r['rmse']:12.6g} {r['w_rmse']:12.6g}{mark}")
    print(f"best: {res.best_setting}, sparsest within one standard error: {res.sparsest_setting}")
    if res.best is not None:
        sup = res.active[res.best][res.active[res.best] >= 0]
        print("descriptor: coefficient +- one standard deviation (share of the fold refits that kept it)")
        for p, j in enumerate(sup):
            print(f"  {int(j):3d}: {res.fits[res.best, j]: .6e} +- {res.errbars[res.best, p]:.2e}  ({res.frequency[j]:.2f})")
    if (res.status == 1).any():
        print(f"{int((res.status == 1).sum())} problems failed")
    pt.free()


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--by", default="Configs", choices=["Groups", "Configs"])
    ap.add_argument("--folds", type=int, default=5)
    ap.add_argument("--method", default="auto", choices=["auto", "device", "host"])
    ap.add_argument("--deletion", default="reference", choices=["reference", "exact"])
    a = ap.parse_args()
    main(a.by, a.folds, a.method, a.deletion)
