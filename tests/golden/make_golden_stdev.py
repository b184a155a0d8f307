"""Generate tests/golden/ta_stdev_reference.npz by RUNNING THE REFERENCE'S OWN ANL solver and its
``Solver._compute_stdev``.

Run in the build container only (needs /root/reference):

    python tests/golden/make_golden_stdev.py

It seeds numpy's global generator, runs the reference's ``ANL`` class through its solver_factory on the Ta golden
matrices (tests/golden/ta_abw.npz, testing rows from ta_reference_fits.npz) with NSAM coefficient samples, and stores the
posterior mean, covariance and samples the class left, and ``_compute_stdev(A, method)`` for all six methods over all
rows (a method that raises is stored as NaN, with its exception name).

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
SEED = 0
NSAM = 20
METHODS = ("sam", "chol", "choleye", "svd", "loop", "fullcov")


def main():
    ParallelTools, Config, solver_factory = import_reference()
    z = np.load(os.path.join(HERE, "ta_abw.npz"))
    f = np.load(os.path.join(HERE, "ta_reference_fits.npz"))
    A, b, w = z["A"], z["b"], z["w"]
    m, K = A.shape
    out = {"seed": np.int64(SEED), "nsam": np.int64(NSAM), "methods": np.array(METHODS)}
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as td:
        os.chdir(td)
        try:
            pt = ParallelTools()
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                cfg = Config(pt, settings("ANL", {"SOLVER": {"nsam": NSAM}}), arguments_lst=["--overwrite"])
            s = solver_factory.solver("ANL", pt, cfg)
            pt.create_shared_array('a', m, K)
            pt.create_shared_array('b', m)
            pt.create_shared_array('w', m)
            pt.shared_arrays['a'].array[:] = A
            pt.shared_arrays['b'].array[:] = b
            pt.shared_arrays['w'].array[:] = w
            pt.fitsnap_dict['Testing'] = [bool(x) for x in f["testing_mask"]]
            np.random.seed(SEED)
            s.perform_fit()
            out["fit"] = np.asarray(s.fit, dtype=np.float64)
            out["cov"] = np.asarray(s.cov, dtype=np.float64)
            out["fit_sam"] = np.asarray(s.fit_sam, dtype=np.float64)
            for meth in METHODS:
                try:
                    with warnings.catch_warnings():
                        warnings.simplefilter("ignore")
                        out[f"stdev_{meth}"] = np.asarray(s._compute_stdev(A, method=meth), dtype=np.float64)
                    out[f"error_{meth}"] = np.array("")
                except Exception as e:  # noqa: BLE001 - recorded, the product must raise the same class
                    out[f"stdev_{meth}"] = np.full(m, np.nan)
                    out[f"error_{meth}"] = np.array(type(e).__name__)
                print(meth, out[f"error_{meth}"], flush=True)
        finally:
            os.chdir(cwd)
    np.savez_compressed(os.path.join(HERE, "ta_stdev_reference.npz"), **out)


if __name__ == "__main__":
    main()
