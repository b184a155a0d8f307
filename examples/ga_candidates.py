"""One generation of a genetic-algorithm weight search on the golden Ta rows, batched (fitsnap_amd.solvers.CandidateFits).

The reference's GA (examples/library/genetic_algorithm/libmod_optimize.py) builds a weight vector per candidate with
update_weights (energy / force / stress weight per group) and runs perform_fit + error_analysis for each.  Here the whole
generation is fitted from per-category statistics and scored from one error pass per 16 candidates.

    python examples/ga_candidates.py [population]
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


def main(population=50):
    z = np.load(os.path.join(ROOT, "tests", "golden", "ta_abw.npz"))
    f = np.load(os.path.join(ROOT, "tests", "golden", "ta_reference_fits.npz"))
    A, b = np.ascontiguousarray(z["A"]), np.ascontiguousarray(z["b"])
    fs = {"Groups": [str(g) for g in f["ea_groups"]], "Testing": f["testing_mask"].tolist(),
          "Row_Type": ["Energy"] * 363 + ["Force"] * 12672 + ["Stress"] * 2178}
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
    t0 = time.perf_counter()
    betas = cf.fit(S)
    tables = cf.errors(betas, S, frames=False)
    dt = time.perf_counter() - t0
    # a fit_and_cost-style score: unweighted energy + force RMSE of the training rows (*ALL rows of the table)
    subs = sorted({(k[1], k[2]) for k in cf.keys})
    pos = {k: i for i, k in enumerate(subs)}
    scores = [tab[1][pos[(False, "Energy")], 2] + tab[1][pos[(False, "Force")], 2] for tab in tables]
    best = int(np.argmin(scores))
    print(f"{population} candidates in {1e3 * dt:.1f} ms ({1e3 * dt / population:.3f} ms each); best #{best}: "
          f"score {scores[best]:.4g}, path {cf.info[best]['path']}, rank {cf.info[best]['rank']}")
    solver.fit = betas[best].copy()                       # then solver._offset() for bzeroflag SNAP, and write_output
    pt.free()


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 50)
