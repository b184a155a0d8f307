"""Noise levels per (group, row type) from the marginal likelihood of the weights
(fitsnap_amd.solvers.CandidateFits.evidence / maximise_evidence).

Synthetic rows: groups whose force targets carry different noise levels.  A GA-style generation of weight candidates (eweight
1e-4 ... 1e4 and a force ratio per group) is the set of starts of a fixed-point ascent of the evidence over log|S| -- no folds,
no pass over the rows, one call per iteration for all candidates.  Under ``scale="fixed"`` the fitted 1 / |S| ARE the noise
standard deviations; the ``noise`` table gives them per category with the effective number of parameters each category
determines.  The winning scales then go to ``fit`` and, as the posterior covariance, to ``prediction_variance``.

    python examples/ga_evidence.py [population] [steps]
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))

from fitsnap_amd.config import Config  # noqa: E402
from fitsnap_amd.parallel_tools import ParallelTools  # noqa: E402
from fitsnap_amd.solvers import CandidateFits, solver_factory  # noqa: E402
from ga_gradient_descent import NOISE, synthetic  # noqa: E402

ENERGY_NOISE = 0.01                                      # of every group's energy rows (ga_gradient_descent.synthetic)


def main(population=32, steps=30):
    A, b, fs = synthetic()
    pt = ParallelTools()
    solver = solver_factory.solver("SVD", pt, Config(pt, {"SOLVER": {"solver": "SVD"}}))
    cf = CandidateFits(solver, A, b, fs_dict=fs)
    groups = sorted(set(fs["Groups"]))
    rng = np.random.default_rng(1)
    cands = []
    for _ in range(population):
        ew = 10.0 ** rng.uniform(-4, 4, len(groups))
        cands.append({g: {"eweight": ew[i], "fweight": ew[i] * 10.0 ** rng.uniform(-3, 3), "vweight": 0.0}
                      for i, g in enumerate(groups)})
    S0 = cf.scales_from_group_weights(cands)
    t0 = time.perf_counter()
    ev0 = cf.evidence(S0, scale="fixed")
    t_ev = time.perf_counter() - t0
    print(f"{population} candidates x {cf.ncat} categories: evidence and exact gradient in {1e3 * t_ev:.1f} ms ({ev0.method} route)")
    t0 = time.perf_counter()
    S, ev, history, converged = cf.maximise_evidence(S0, scale="fixed", steps=steps)
    t_max = time.perf_counter() - t0
    print(f"{len(history) - 1} fixed-point iterations from every candidate: {t_max:.2f} s, {int(converged.sum())} of {population} "
          f"converged")
    print(f"log evidence   before {np.nanmax(history[0]):12.2f} (best)   after {np.nanmax(history[-1]):12.2f} (best) "
          f"{np.nanmin(history[-1]):12.2f} (worst)")
    best = int(np.nanargmax(history[-1]))
    print(f"winning start: candidate {best}.  category, rows, effective parameters, fitted noise sd = 1 / |S|, sqrt(noise), true sd")
    for c, (g, _, rt) in enumerate(cf.keys):
        true = ENERGY_NOISE if rt == "Energy" else NOISE[int(g[1:])]
        n_c = int(np.count_nonzero(cf.cat == c))
        print(f"  {g} {rt:6s} {n_c:5d}  {ev.dof[best, c]:7.2f}  {1 / abs(S[best, c]):10.4g}  "
              f"{np.sqrt(ev.noise[best, c]):10.4g}  {true:8.3g}")
    # the winning scales as weights of a fit, and as the posterior of the predictive variance
    beta = cf.fit(S[best:best + 1])[0]
    G = cf.candidate_statistics(0)[0]
    solver.fit = beta.copy()
    solver.use_covariance(np.linalg.inv(G))                # unit noise scale: the weights are 1 / sd
    pv = solver.prediction_variance(A, categories=fs["Groups"])
    print("mean predictive sd of the rows per group under the winning weights:")
    for g, v in zip(pv["keys"], pv["cat_mean"]):
        print(f"  {g}  {np.sqrt(v):.4g}")
    assert np.all(np.diff(history, axis=0) >= 0) and np.max(np.abs(beta - ev.beta[best])) <= 1e-6 * np.max(np.abs(beta))
    pt.free()


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 32, int(sys.argv[2]) if len(sys.argv) > 2 else 30)
