"""Which configurations move the coefficients, and how uncertain are the coefficients when the rows of one configuration
share an error?  Influence and cluster-robust covariances of a RIDGE fit on the GPU (Solver.influence).

Synthetic rows in configurations whose targets carry a per-configuration random effect next to the i.i.d. noise, as force
and stress rows of one structure share a model-form error, and one configuration with a gross error.  After one fit:
Cook's distance of every configuration from the exact leave-one-configuration-out algebra (no refit), the standard errors
of the coefficients under the classical covariance sigma^2 (G + alpha I)^-1, the cluster-robust one (CR1) and the
delete-one-configuration jackknife, and the predictive variance of a few rows under the classical and the robust
covariance.

    python examples/influence_covariance.py [--rows 20000] [--columns 16] [--effect 0.5]
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


def main(rows=20000, K=16, effect=0.5):
    rng = np.random.default_rng(0)
    sizes = []
    while sum(sizes) < rows:
        sizes.append(int(rng.integers(5, 60)))
    m, U = sum(sizes), len(sizes)
    cfg = np.repeat(np.arange(U), sizes)
    A = (rng.standard_normal((U, K))[cfg] + rng.standard_normal((m, K))) / np.sqrt(2.0)
    b = A @ rng.standard_normal(K) + effect * rng.standard_normal(U)[cfg] + 0.1 * rng.standard_normal(m)
    b[cfg == 7] += 3.0                                            # one configuration with a gross error
    labels = {"Configs": [f"cfg{c}" for c in cfg], "Groups": [f"g{c % 3}" for c in cfg], "Testing": [False] * m,
              "Row_Type": ["Force"] * m}
    pt = ParallelTools()
    s = solver_factory.solver("RIDGE", pt, Config(pt, {"SOLVER": {"solver": "RIDGE"}, "RIDGE": {"alpha": 1e-8}}))
    s.perform_fit(A, b, np.ones(m), fs_dict=labels)
    res = s.influence(kinds=("cr1", "jack"), fs_dict=labels, b=b, w=np.ones(m))
    print(f"RIDGE on {m} x {K} rows in {U} configurations, sigma^2 = {res.noise:.4f}, {res.unidentifiable} not identifiable")
    print("configurations by Cook's distance:")
    print(res.units.sort_values("cook", ascending=False).head(5).to_string(index=False))
    print("standard errors of the coefficients:")
    print(res.stderr.to_string(float_format=lambda x: f"{x:.4g}"))
    first = np.ascontiguousarray(A[:5])
    s.use_covariance(res.cov["classical"])
    classical = s.prediction_variance(a=first, want_preds=False)["var"]
    s.use_covariance(res.cov["cr1"])
    robust = s.prediction_variance(a=first, want_preds=False)["var"]
    print("predictive variance of the first rows, classical:", np.array2string(classical, precision=4))
    print("                               cluster-robust (CR1):", np.array2string(robust, precision=4))
    pt.free()


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--rows", type=int, default=20000)
    ap.add_argument("--columns", type=int, default=16)
    ap.add_argument("--effect", type=float, default=0.5)
    a = ap.parse_args()
    main(a.rows, a.columns, a.effect)
