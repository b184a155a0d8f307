"""A fit that a few percent of wrong rows do not pull: the ROBUST solver (Solver.robust_fit, M-estimator by IRLS on the GPU).

Synthetic energy / force / stress rows in configurations; the noise of the three row types differs by three decades and the
weights undo most of it, as a FitSNAP group-weight table would.  --outliers of the rows are simply wrong (20 - 200 sigma
off: unconverged DFT, a flipped force component), and they sit in a --bad share of the configurations.  Printed: the
coefficient error of the least-squares fit (RIDGE) next to the robust fits of the three losses, the per-row-type scales and
counts of the last iteration, and the suspect-configuration table -- what one would otherwise dig out of error_analysis by
hand.

    python examples/robust_fit.py [--rows 30000] [--columns 31] [--outliers 0.05] [--bad 0.1]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from fitsnap_amd.config import Config  # noqa: E402
from fitsnap_amd.parallel_tools import ParallelTools  # noqa: E402
from fitsnap_amd.solvers import robust, solver_factory  # noqa: E402


def main(rows=30000, K=31, outliers=0.05, bad=0.1):
    rng = np.random.default_rng(0)
    per_cfg = 25
    ncfg = rows // per_cfg
    m = ncfg * per_cfg
    cfg = np.repeat(np.arange(ncfg), per_cfg)
    kind = np.tile(np.array([0] + [1] * 18 + [2] * 6), ncfg)              # 1 energy, 18 force, 6 stress rows per configuration
    sigma = np.array([1e-3, 5e-2, 2.0])[kind]
    A = rng.standard_normal((m, K)) * 10.0 ** rng.uniform(-1, 1, K)
    truth = rng.standard_normal(K)
    b = A @ truth + sigma * rng.standard_normal(m)
    w = np.array([100.0, 1.0, 1e-2])[kind]
    bad_cfg = rng.choice(ncfg, max(1, int(bad * ncfg)), replace=False)
    pool = np.flatnonzero(np.isin(cfg, bad_cfg))
    wrong = rng.choice(pool, min(len(pool), int(outliers * m)), replace=False)
    b[wrong] += rng.choice([-1.0, 1.0], len(wrong)) * rng.uniform(20, 200, len(wrong)) * sigma[wrong]
    pt = ParallelTools()
    pt.create_shared_array("a", m, K)
    pt.create_shared_array("b", m)
    pt.create_shared_array("w", m)
    pt.shared_arrays["a"].array[:] = A
    pt.shared_arrays["b"].array[:] = b
    pt.shared_arrays["w"].array[:] = w
    pt.fitsnap_dict = {"Configs": [f"cfg{c}" for c in cfg], "Groups": [f"g{c % 3}" for c in cfg], "Testing": [False] * m,
                       "Row_Type": [("Energy", "Force", "Stress")[k] for k in kind]}
    ls = solver_factory.solver("RIDGE", pt, Config(pt, {"SOLVER": {"solver": "RIDGE"}}))
    ls.perform_fit()
    err_ls = float(np.max(np.abs(ls.fit - truth)))
    print(f"{m} x {K} rows in {ncfg} configurations, {len(wrong)} wrong rows in {len(bad_cfg)} of them")
    print(f"least squares (RIDGE)   max |beta - truth| = {err_ls:.3e}")
    s = None
    for loss in robust.DEFAULT_TUNE:
        s = solver_factory.solver("ROBUST", pt, Config(pt, {"SOLVER": {"solver": "ROBUST"}, "ROBUST": {"loss": loss}}))
        s.perform_fit()
        res = s.robust
        err = float(np.max(np.abs(s.fit - truth)))
        print(f"ROBUST {loss:9s}        max |beta - truth| = {err:.3e} ({err / err_ls:.3f} x least squares), "
              f"{res.iterations} iterations, converged {res.converged}")
    res = s.robust
    print(f"last iteration of the {res.loss} fit, per row type:")
    for key, sc, row in zip(res.classes, res.scales[-1], res.tables[-1]):
        print(f"  {key:7s} scale {sc:.4e}   n {int(row[0]):7d}   down-weighted {int(row[1]):6d}   rejected {int(row[2]):6d}   "
              f"mean omega {row[3] / max(row[0], 1):.4f}")
    tab = res.table(by="Configs")
    top = tab.head(len(bad_cfg))
    hit = len(set(top["Configs"]) & {f"cfg{c}" for c in bad_cfg})
    print(f"suspect configurations (lowest mean omega first); {hit} of the first {len(bad_cfg)} are planted ones:")
    print(tab.head(12).to_string(index=False, float_format=lambda x: f"{x:.4f}"))
    pt.free()


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--rows", type=int, default=30000)
    ap.add_argument("--columns", type=int, default=31)
    ap.add_argument("--outliers", type=float, default=0.05)
    ap.add_argument("--bad", type=float, default=0.1)
    a = ap.parse_args()
    main(a.rows, a.columns, a.outliers, a.bad)
