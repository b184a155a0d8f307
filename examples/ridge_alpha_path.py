"""Choosing [RIDGE] alpha by exact leave-one-group-out error on the golden Ta rows, on the GPU (Solver.ridge_path).

One RIDGE fit, then for every alpha of a grid every training row is predicted by the refit without the rows of its group
(ea_groups of ta_reference_fits.npz): the *ALL rows of the table per alpha, the alpha with the smallest weighted LOO error
and the fit at that alpha next to the fit at the configured one.

    python examples/ridge_alpha_path.py [--by Groups|Configs] [--method auto|refit|woodbury]

The fixture has no configuration labels; --by Configs takes blocks of 7 consecutive rows as stand-ins.
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


def main(by="Groups", method="auto"):
    z = np.load(os.path.join(ROOT, "tests", "golden", "ta_abw.npz"))
    f = np.load(os.path.join(ROOT, "tests", "golden", "ta_reference_fits.npz"))
    A, b, w = (np.ascontiguousarray(z[k]) for k in ("A", "b", "w"))
    m = len(b)
    fs = {"Groups": [str(g) for g in f["ea_groups"]], "Testing": [False] * m, "Row_Type": ROW_TYPE,
          "Configs": [f"c{i // 7}" for i in range(m)]}
    pt = ParallelTools()
    s = solver_factory.solver("RIDGE", pt, Config(pt, {"SOLVER": {"solver": "RIDGE"}, "RIDGE": {"alpha": 1e-8}}))
    s.keep_resident = True
    s.perform_fit(A, b, w, fs_dict=fs)
    alphas = np.concatenate([[0.0], np.logspace(-10, 2, 13)])
    res = s.ridge_path(alphas, by=by, fs_dict=fs, b=b, w=w, method=method)
    print(f"leave-one-{by[:-1].lower()}-out error of the ridge fit on {m} x {A.shape[1]} Ta rows, {len(alphas)} alphas")
    print(f"{'alpha':>10} {'rows':>7} {'mae':>12} {'rmse':>12} {'w_rmse':>12} {'not identifiable':>17}")
    for q, alpha in enumerate(alphas):
        r = res.table.loc[(float(alpha), "*ALL")]
        print(f"{alpha:10.3g} {int(r['ncount']):7d} {r['mae']:12.6g} {r['rmse']:12.6g} {r['w_rmse']:12.6g} "
              f"{int(res.unidentifiable[q]):17d}   *ALL")
    print(f"best alpha: {res.best_alpha:g} (configured: 1e-08)")
    print(f"largest change of a coefficient from the configured fit: {np.max(np.abs(res.fits[res.best] - np.asarray(s.fit).reshape(-1))):.3g}")
    pt.free()


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--by", default="Groups", choices=["Groups", "Configs"])
    ap.add_argument("--method", default="auto", choices=["auto", "refit", "woodbury"])
    a = ap.parse_args()
    main(a.by, a.method)
