"""Generate tests/golden/ta_mcmc_reference.npz by RUNNING THE REFERENCE'S OWN MCMC solver.

Run in the build container only (needs the reference checkout):

    python tests/golden/make_golden_mcmc.py

For each case below it seeds numpy's global generator, runs the reference's ``MCMC`` class (mcmc.py ``amcmc``) through
its solver_factory on the Ta rows of tests/golden/ta_abw.npz (shared arrays, ``pt.fitsnap_dict['Testing']``) and stores:
the settings, the testing mask, the accept pattern (one bool per step), every STRIDE-th sample, ``cmode`` / ``pmode``,
``fit_sam``, the unique-sample weights, the acceptance rate and the next ``np.random.random_sample()`` after the fit (where
the fit left the global generator).  ``amcmc`` is wrapped only to record what it returns.

Only data is written: no reference source text is copied.
"""
from __future__ import annotations

import os
import sys
import tempfile
import warnings

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import import_reference, settings  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
STRIDE = 10
SEED = 7
NMCMC = 3000
# (tag, gamma, sigma, testing row stride (0 = none), apply_transpose)
CASES = [
    ("train", 0.01, 0.1, 0, 0),
    ("testing", 0.03, 0.2, 5, 0),
    ("transpose", 0.01, 0.1, 0, 1),
]


def testing_mask(m, stride):
    t = np.zeros(m, dtype=bool)
    if stride:
        t[2::stride] = True
    return t


def main():
    ParallelTools, Config, solver_factory = import_reference()
    from fitsnap3lib.solvers import mcmc as ref_mcmc

    z = np.load(os.path.join(HERE, "ta_abw.npz"))
    A, b, w = z["A"], z["b"], z["w"]
    m, K = A.shape

    captured = {}
    real_amcmc = ref_mcmc.amcmc

    def recording_amcmc(*args, **kw):
        out = real_amcmc(*args, **kw)
        captured["out"] = out
        return out

    ref_mcmc.amcmc = recording_amcmc
    out = {"stride": np.int64(STRIDE), "seed": np.int64(SEED), "nmcmc": np.int64(NMCMC),
           "tags": np.array([c[0] for c in CASES])}
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as td:
        os.chdir(td)
        try:
            for tag, gamma, sigma, tstride, transpose in CASES:
                pt = ParallelTools()
                extra = {"SOLVER": {"mcmc_num": NMCMC, "mcmc_gamma": gamma, "mcmc_sigma": sigma}}
                if transpose:
                    extra["EXTRAS"] = {"apply_transpose": 1}
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    cfg = Config(pt, settings("MCMC", extra), arguments_lst=["--overwrite"])
                s = solver_factory.solver("MCMC", pt, cfg)
                pt.create_shared_array('a', m, K)
                pt.create_shared_array('b', m)
                pt.create_shared_array('w', m)
                pt.shared_arrays['a'].array[:] = A
                pt.shared_arrays['b'].array[:] = b
                pt.shared_arrays['w'].array[:] = w
                testing = testing_mask(m, tstride)
                pt.fitsnap_dict['Testing'] = testing.tolist()
                np.random.seed(SEED)
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")       # multivariate_normal's PSD warning on the zero covariance
                    s.perform_fit()
                nxt = np.random.random_sample()
                samples, cmode, pmode, acc_rate, _, _, weights, _ = captured["out"]
                change = np.concatenate([[0], np.cumsum(weights)[:-1]]).astype(np.int64)
                accepted = np.zeros(NMCMC - 1, dtype=bool)
                accepted[change[1:] - 1] = True
                out[f"{tag}_gamma"] = np.float64(gamma)
                out[f"{tag}_sigma"] = np.float64(sigma)
                out[f"{tag}_transpose"] = np.int64(transpose)
                out[f"{tag}_testing"] = testing
                out[f"{tag}_accepted"] = accepted
                out[f"{tag}_samples"] = samples[::STRIDE].copy()
                out[f"{tag}_last"] = samples[-1].copy()
                out[f"{tag}_cmode"] = np.asarray(cmode, dtype=np.float64)
                out[f"{tag}_pmode"] = np.float64(pmode)
                out[f"{tag}_fit"] = np.asarray(s.fit, dtype=np.float64)
                out[f"{tag}_fit_sam"] = np.asarray(s.fit_sam, dtype=np.float64)
                out[f"{tag}_weights"] = np.asarray(weights, dtype=np.float64)
                out[f"{tag}_acc_rate"] = np.float64(acc_rate)
                out[f"{tag}_next_uniform"] = np.float64(nxt)
                print(f"{tag}: acceptance {acc_rate:.4f}, pmode {pmode:.6f}", flush=True)
        finally:
            os.chdir(cwd)
            ref_mcmc.amcmc = real_amcmc
    np.savez_compressed(os.path.join(HERE, "ta_mcmc_reference.npz"), **out)


if __name__ == "__main__":
    main()
