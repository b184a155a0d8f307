"""One generation of a genetic-algorithm weight search on the golden Ta rows, scored on rows the fits have NOT seen
(fitsnap_amd.solvers.CandidateFits.cross_validate).

The reference's GA (examples/library/genetic_algorithm/libmod_optimize.py) scores a candidate by
etot_weight * rmse_E + ftot_weight * rmse_F of the rows its fit was made on (fit_and_cost).  Here the configurations are dealt
into folds, every candidate is refitted with each fold left out -- all refits from one pass of per-(fold, category)
statistics, solved on the GPU -- and the same objective is taken over the held-out rows.  The ranking under both scores is
printed side by side.

    python examples/ga_cross_validated.py [population] [folds]
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from fitsnap_amd.config import Config  # noqa: E402
from fitsnap_amd.parallel_tools import ParallelTools  # noqa: E402
from fitsnap_amd.solvers import CandidateFits, solver_factory  # noqa: E402

ETOT_WEIGHT, FTOT_WEIGHT = 1.0, 1.0


def main(population=32, folds=5):
    z = np.load(os.path.join(ROOT, "tests", "golden", "ta_abw.npz"))
    f = np.load(os.path.join(ROOT, "tests", "golden", "ta_reference_fits.npz"))
    A, b = np.ascontiguousarray(z["A"]), np.ascontiguousarray(z["b"])
    m = len(b)
    # the golden matrices carry no configuration labels: blocks of 7 rows stand in for them
    fs = {"Groups": [str(g) for g in f["ea_groups"]], "Testing": f["testing_mask"].tolist(),
          "Row_Type": ["Energy"] * 363 + ["Force"] * 12672 + ["Stress"] * 2178, "Configs": [f"c{i // 7}" for i in range(m)]}
    pt = ParallelTools()
    solver = solver_factory.solver("SVD", pt, Config(pt, {"SOLVER": {"solver": "SVD"}}))
    cf = CandidateFits(solver, A, b, fs_dict=fs)          # w0 = 1: S holds update_weights' absolute weights
    groups = sorted(set(fs["Groups"]))
    rng = np.random.default_rng(0)
    cands = []
    for _ in range(population):                           # update_weights' table: eweight, eweight * ratio per group
        ew = 10.0 ** rng.uniform(-4, 4, len(groups))
        cands.append({g: {"eweight": ew[i], "fweight": ew[i] * 10.0 ** rng.uniform(-3, 3),
                          "vweight": ew[i] * 10.0 ** rng.uniform(-3, 3)} for i, g in enumerate(groups)})
    S = cf.scales_from_group_weights(cands)
    # in-sample: fit_and_cost's objective on the training rows (*ALL rows of the error tables)
    t0 = time.perf_counter()
    betas = cf.fit(S)
    tables = cf.errors(betas, S, frames=False)
    t_in = time.perf_counter() - t0
    subs = sorted({(k[1], k[2]) for k in cf.keys})
    pos = {k: i for i, k in enumerate(subs)}
    in_sample = np.array([ETOT_WEIGHT * tab[1][pos[(False, "Energy")], 2] + FTOT_WEIGHT * tab[1][pos[(False, "Force")], 2]
                          for tab in tables])
    # held-out: the same objective over rows whose configuration the refit did not see
    t0 = time.perf_counter()
    cv = cf.cross_validate(S, folds=folds, by="Configs")
    held_out = cv.cost({"Energy": ETOT_WEIGHT, "Force": FTOT_WEIGHT})
    t_cv = time.perf_counter() - t0
    print(f"{population} candidates: in-sample fit + errors {1e3 * t_in:.1f} ms; {folds}-fold cross-validation "
          f"({population * folds} refits) {1e3 * t_cv:.1f} ms; failed refits: {int(np.count_nonzero(cv.status))}")
    order_in, order_cv = np.argsort(in_sample), np.argsort(np.where(np.isnan(held_out), np.inf, held_out))
    rank_cv = {int(p): r for r, p in enumerate(order_cv)}
    print("rank  candidate  in-sample cost  held-out cost  rank held-out")
    for r, p in enumerate(order_in[:10]):
        print(f"{r:4d}  {int(p):9d}  {in_sample[p]:14.6g}  {held_out[p]:13.6g}  {rank_cv[int(p)]:13d}")
    best = int(order_cv[0])
    print(f"best held-out: candidate {best} (in-sample rank {int(np.flatnonzero(order_in == best)[0])}), "
          f"cost {held_out[best]:.6g}")
    print(cv.tables()[best].loc["*ALL"])
    solver.fit = betas[best].copy()                       # the fit on all training rows of the chosen weights
    pt.free()


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 32, int(sys.argv[2]) if len(sys.argv) > 2 else 5)
