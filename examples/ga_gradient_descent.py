"""A GA population as the starts of a first-order descent on the cross-validated cost
(fitsnap_amd.solvers.CandidateFits.cross_validate_gradient / descend_weights).

Synthetic rows: groups whose targets carry different noise levels, so that the best weights are NOT equal -- a noisy group
should count for less.  A GA-style population of weight candidates (eweight 1e-4 ... 1e4 and a force ratio per group) is scored
on held-out configurations, then every candidate takes 20 Armijo steps down the exact gradient of that score over log|S|,
all candidates at once: one gradient call per iteration, one cross-validation call per line-search round.

    python examples/ga_gradient_descent.py [population] [steps]
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

WEIGHTS = {"Energy": 1.0, "Force": 0.3}
NOISE = [0.01, 0.03, 0.1, 0.3, 1.0, 3.0]                  # per group: the last groups are nearly useless


def synthetic(K=40, configs_per_group=60, seed=0):
    """(A, b, fs_dict): per configuration one energy row and 11 force rows; the force targets of group g carry NOISE[g]."""
    rng = np.random.default_rng(seed)
    truth = rng.standard_normal(K)
    rows, targets, groups, types, configs = [], [], [], [], []
    for g, noise in enumerate(NOISE):
        for c in range(configs_per_group):
            a = rng.standard_normal((12, K))
            t = a @ truth
            t[0] += 0.01 * rng.standard_normal()
            t[1:] += noise * rng.standard_normal(11)
            rows.append(a)
            targets.append(t)
            groups += [f"g{g}"] * 12
            types += ["Energy"] + ["Force"] * 11
            configs += [f"g{g}c{c}"] * 12
    m = len(groups)
    fs = {"Groups": groups, "Testing": [False] * m, "Row_Type": types, "Configs": configs}
    return np.ascontiguousarray(np.vstack(rows)), np.concatenate(targets), fs


def main(population=32, steps=20):
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
    r = cf.cross_validate_gradient(S0, WEIGHTS, folds=5, by="Configs")
    t_grad = time.perf_counter() - t0
    print(f"{population} candidates x {cf.ncat} categories: cost and exact gradient in {1e3 * t_grad:.1f} ms "
          f"(finite differences: {2 * cf.ncat} cross-validations per candidate batch)")
    t0 = time.perf_counter()
    S, history, taken = cf.descend_weights(S0, WEIGHTS, steps=steps, folds=5, by="Configs")
    t_desc = time.perf_counter() - t0
    print(f"{steps} descent steps from every candidate: {t_desc:.2f} s, {int(np.count_nonzero(taken))} accepted steps")
    print("held-out cost   before        after")
    print(f"  best        {np.nanmin(history[0]):10.5f}   {np.nanmin(history[-1]):10.5f}")
    print(f"  median      {np.nanmedian(history[0]):10.5f}   {np.nanmedian(history[-1]):10.5f}")
    print(f"  worst       {np.nanmax(history[0]):10.5f}   {np.nanmax(history[-1]):10.5f}")
    best = int(np.nanargmin(history[-1]))
    print(f"best start after the descent: candidate {best}; its force scales per group (noise level):")
    for c, (g, _, rt) in enumerate(cf.keys):
        if rt == "Force":
            print(f"  {g} (noise {NOISE[int(g[1:])]:4.2f})  {abs(S0[best, c]):10.3g} -> {abs(S[best, c]):10.3g}")
    assert np.all(np.diff(history, axis=0) <= 0) and r.cost.shape == (population,)
    pt.free()


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 32, int(sys.argv[2]) if len(sys.argv) > 2 else 20)
