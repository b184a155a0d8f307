"""Generate tests/golden/ta_merr_reference.npz by RUNNING THE REFERENCE'S OWN MERR solver.

Run in the build container only (needs /root/reference):

    python tests/golden/make_golden_merr.py

For each case below it seeds numpy's global generator, runs the reference's ``MERR`` class (merr.py + lreg.py
``lreg_merr``, BFGS with finite differences) through its solver_factory on the Ta golden matrices, and stores the
settings, the reference's final parameter vector (coefficients then sigmas, as returned by its BFGS), ``mean`` /
``covariance`` as written by the class, the data variance it used, and the log-posterior at the final vector evaluated
with the reference's own ``logpost_emb``.

Row subset: every ROW_STRIDE-th row of tests/golden/ta_abw.npz (all of them training rows).  The full 15 213 rows take
about 7 minutes per case on a few CPU cores; the subset keeps the five cases to a few minutes.

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
ROW_STRIDE = 5
SEED = 0
# (tag, merr_method, merr_mult, merr_cfs)
CASES = [
    ("iid_add", "iid", 0, "all"),
    ("iid_mult", "iid", 1, "all"),
    ("abc_add", "abc", 0, "all"),
    ("abc_mult", "abc", 1, "all"),
    ("abc_add_cfs", "abc", 0, "0 3 7 12 20 30"),
]


def main():
    ParallelTools, Config, solver_factory = import_reference()
    from fitsnap3lib.solvers import lreg as ref_lreg

    z = np.load(os.path.join(HERE, "ta_abw.npz"))
    A, b, w = z["A"][::ROW_STRIDE].copy(), z["b"][::ROW_STRIDE].copy(), z["w"][::ROW_STRIDE].copy()
    m, K = A.shape

    captured = {}
    real_minimize = ref_lreg.minimize

    def recording_minimize(fun, x0, args=(), **kw):
        res = real_minimize(fun, x0, args=args, **kw)
        captured["x"] = np.array(res.x, dtype=np.float64)
        captured["nfev"] = int(res.nfev)
        captured["params"] = dict(args[1])
        return res

    ref_lreg.minimize = recording_minimize
    out = {"row_stride": np.int64(ROW_STRIDE), "seed": np.int64(SEED), "tags": np.array([c[0] for c in CASES])}
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as td:
        os.chdir(td)
        try:
            for tag, method, mult, cfs in CASES:
                pt = ParallelTools()
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    cfg = Config(pt, settings("MERR", {"SOLVER": {"merr_method": method, "merr_mult": mult,
                                                                  "merr_cfs": cfs, "nsam": 0}}),
                                 arguments_lst=["--overwrite"])
                s = solver_factory.solver("MERR", pt, cfg)
                pt.create_shared_array('a', m, K)
                pt.create_shared_array('b', m)
                pt.create_shared_array('w', m)
                pt.shared_arrays['a'].array[:] = A
                pt.shared_arrays['b'].array[:] = b
                pt.shared_arrays['w'].array[:] = w
                pt.fitsnap_dict['Testing'] = [False] * m
                np.random.seed(SEED)
                s.perform_fit()
                p = captured["params"]
                x = captured["x"]
                L = float(ref_lreg.logpost_emb(x, **p))
                out[f"{tag}_method"] = np.array(method)
                out[f"{tag}_mult"] = np.int64(mult)
                out[f"{tag}_cfs"] = np.array(cfs)
                out[f"{tag}_x"] = x
                out[f"{tag}_mean"] = np.load("mean.npy")
                out[f"{tag}_cov"] = np.load("covariance.npy")
                out[f"{tag}_datavar"] = np.float64(p["datavar"])
                out[f"{tag}_logpost"] = np.float64(L)
                out[f"{tag}_nfev"] = np.int64(captured["nfev"])
                print(f"{tag}: L = {L:.6f}, {captured['nfev']} evaluations", flush=True)
        finally:
            os.chdir(cwd)
            ref_lreg.minimize = real_minimize
    np.savez_compressed(os.path.join(HERE, "ta_merr_reference.npz"), **out)


if __name__ == "__main__":
    main()
