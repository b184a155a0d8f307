"""Choosing how many basis functions to keep, and which, by grouped cross-validation on the golden Ta rows, on the GPU
(Solver.omp_path), then refitting with that many terms and writing the sparse coefficients.

One OMP fit, then ONE pass over the rows for the statistics of every fold and, for every fold left out, a greedy forward
selection on "total minus fold": the held-out error after every step with its standard error over the folds, the size with
the smallest error and the fewest terms within one standard error of it, and how often the folds agree on each column.  The
solver is then re-configured with ``sparsest_terms`` and fitted again; the kept columns and their coefficients go to a text
file.

    python examples/omp_sparse_path.py [--by Groups|Configs] [--folds F] [--criterion ols|omp] [--method auto|device|host] [--out FILE]

The fixture has no configuration labels; --by Configs takes blocks of 7 consecutive rows as stand-ins and deals them into
--folds folds.
"""
import argparse
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from fitsnap_amd.config import Config  # noqa: E402
from fitsnap_amd.parallel_tools import ParallelTools  # noqa: E402
from fitsnap_amd.solvers import solver_factory  # noqa: E402

ROW_TYPE = ["Energy"] * 363 + ["Force"] * 12672 + ["Stress"] * 2178


def main(by="Groups", folds=5, criterion="ols", method="auto", out=None):
    z = np.load(os.path.join(ROOT, "tests", "golden", "ta_abw.npz"))
    f = np.load(os.path.join(ROOT, "tests", "golden", "ta_reference_fits.npz"))
    A, b, w = (np.ascontiguousarray(z[k]) for k in ("A", "b", "w"))
    m, K = A.shape
    pt = ParallelTools()
    cfg = Config(pt, {"SOLVER": {"solver": "OMP"}, "OMP": {"criterion": criterion}})
    s = solver_factory.solver("OMP", pt, cfg)
    for name, arr in (("a", A), ("b", b), ("w", w)):
        pt.create_shared_array(name, m, K if name == "a" else 1)
        pt.shared_arrays[name].array[:] = arr
    pt.fitsnap_dict.update({"Groups": [str(g) for g in f["ea_groups"]], "Testing": [False] * m, "Row_Type": ROW_TYPE,
                            "Configs": [f"c{i // 7}" for i in range(m)]})
    s.perform_fit()                                       # [OMP] terms unset: every column, the plain least-squares fit
    dense = s.fit.copy()
    res = s.omp_path(K, criterion=criterion, folds=None if by == "Groups" else folds, by=by, method=method)
    nfolds = len(set(res.fold_of_unit.values()))
    print(f"{nfolds}-fold cross-validation (by {by}) of greedy selection ({criterion}) on {m} x {K} Ta rows")
    print(f"{'terms':>6} {'column':>7} {'train sse':>12} {'cv error':>12} {'+- se':>10}")
    for i, t in enumerate(res.terms):
        mark = " <- best" if i == res.best else (" <- fewest within one se" if i == res.sparsest else "")
        print(f"{t:6d} {int(res.order[i]):7d} {res.train_sse[i]:12.6g} {res.cv_error[i]:12.6g} {res.cv_se[i]:10.3g}{mark}")
    print(res.table.xs("*ALL", level="Row_Type").to_string())
    agreed = np.flatnonzero(res.frequency == 1.0)
    print(f"best: {res.best_terms} terms; fewest within one standard error: {res.sparsest_terms}; columns every fold chose "
          f"within the best size: {agreed.tolist()}")
    # refit with the chosen size
    cfg.sections["OMP"].terms = int(res.sparsest_terms)
    s.perform_fit()
    kept = np.flatnonzero(s.fit)
    assert kept.size == res.sparsest_terms and sorted(kept.tolist()) == sorted(res.order[:res.sparsest_terms].tolist())
    print(f"refit with {kept.size} of {K} columns: weighted training sse {s.path[-1, 0]:.6g} (all columns: {res.train_sse[-1]:.6g}); "
          f"largest coefficient change on the kept columns {np.max(np.abs(s.fit[kept] - dense[kept])):.3g}")
    out = out or os.path.join(tempfile.mkdtemp(prefix="omp_sparse_"), "sparse_coefficients.txt")
    with open(out, "w") as fh:
        fh.write(f"# {kept.size} of {K} columns kept by {criterion} selection, in the order they were chosen: column coefficient\n")
        for j in s.order[s.order >= 0]:
            fh.write(f"{int(j)} {s.fit[j]:.16e}\n")
    print(f"wrote {out}")
    pt.free()


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--by", default="Groups", choices=["Groups", "Configs"])
    ap.add_argument("--folds", type=int, default=5)
    ap.add_argument("--criterion", default="ols", choices=["ols", "omp"])
    ap.add_argument("--method", default="auto", choices=["auto", "device", "host"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    main(a.by, a.folds, a.criterion, a.method, a.out)
