"""Worker of tests/test_gpu_spectral_path.py: one rank of a spectral-path run (peer-to-peer transport; the ranks may share one
GPU), launched with RANK / WORLD_SIZE / LOCAL_RANK / FSNAP_COMM_FILE / FSNAP_DIST_TRANSPORT in the environment.  Row i lives on
rank i % world, so every configuration spans the ranks; every rank fits RIDGE on its shared rows and calls spectral_path().
Writes what the rank got to <outdir>/spectral_rank<r>.npz."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

ALPHAS, RCONDS = [0.0, 1e-6, 1e-2], [0.0, 1e-3]


def rows():
    import bcs_cases as cs

    A, b, w, conf, cls = cs.rows(31, 31, per=30)
    testing = (np.arange(len(b)) % 10 == 3).tolist()
    labels = {"Configs": [f"c{i:03d}" for i in conf], "Groups": [f"g{i % 4}" for i in conf], "Testing": testing,
              "Row_Type": [("Energy", "Force", "Stress")[k] for k in cls]}
    return np.array(A), np.array(b), np.array(w), labels


def path_of(solver):
    return solver.spectral_path(ALPHAS, RCONDS, folds=4, seed=3, method="device")


def main(outdir):
    from fitsnap_amd.config import Config
    from fitsnap_amd.parallel_tools import ParallelTools
    from fitsnap_amd.solvers import solver_factory

    pt = ParallelTools(comm="rccl")
    rank, world = pt._rank, pt._size
    A, b, w, labels = rows()
    mine = np.flatnonzero(np.arange(len(b)) % world == rank)
    pt.create_shared_array("a", len(mine), A.shape[1])
    pt.create_shared_array("b", len(mine))
    pt.create_shared_array("w", len(mine))
    pt.shared_arrays["a"].array[:] = A[mine]
    pt.shared_arrays["b"].array[:] = b[mine]
    pt.shared_arrays["w"].array[:] = w[mine]
    local = {k: [v[i] for i in mine] for k, v in labels.items()}
    pt.fitsnap_dict = dict(local)
    pt.local_lists = dict(local)
    s = solver_factory.solver("RIDGE", pt, Config(pt, {"SOLVER": {"solver": "RIDGE"}}))
    s.perform_fit()
    res = path_of(s)
    np.savez(os.path.join(outdir, f"spectral_rank{rank}.npz"), rank=res.rank, status=res.status, fits=res.fits, dof=res.dof,
             eigenvalues=res.eigenvalues, table=res.table.to_numpy(dtype=float),
             index=np.array([str(x) for x in res.table.index]), cv_error=res.cv_error, cv_se=res.cv_se, best=res.best,
             simplest=res.simplest, folds=np.array([f"{k}={v}" for k, v in sorted(res.fold_of_unit.items())]))
    pt.free()


if __name__ == "__main__":
    main(sys.argv[1])
