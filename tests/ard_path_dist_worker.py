"""Worker of tests/test_gpu_ard_path.py: one rank of an ARD-path run (peer-to-peer transport; the ranks may share one GPU),
launched with RANK / WORLD_SIZE / LOCAL_RANK / FSNAP_COMM_FILE / FSNAP_DIST_TRANSPORT in the environment (or WORLD_SIZE = 1
with FSNAP_FORCE_MULTI = 1: the collective code paths in a communicator of one rank).  Row i lives on rank i % world, so every
configuration spans the ranks; every rank fits ARD on its shared rows and calls ard_path().  Writes what the rank got to
<outdir>/ard_rank<r>.npz."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SIZES = [12 + (7 * c) % 40 for c in range(30)]
LOGCUTS = [0.3, 1.0, 2.0, 3.0]


def rows():
    from loco_cases import config_rows

    return config_rows(9, 31, SIZES, testing_frac=0.1)


def path_of(solver):
    return solver.ard_path(LOGCUTS, folds=4, seed=3)


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
    s = solver_factory.solver("ARD", pt, Config(pt, {"SOLVER": {"solver": "ARD"}}))
    s.perform_fit()
    res = path_of(s)
    np.savez(os.path.join(outdir, f"ard_rank{rank}.npz"), fits=res.fits, lambdas=res.lambdas, iterations=res.iterations,
             status=res.status, alpha_=res.alpha_, table=res.table.to_numpy(dtype=float),
             index=np.array([str(x) for x in res.table.index]), cv_error=res.cv_error, cv_se=res.cv_se, best=res.best,
             sparsest=res.sparsest, folds=np.array([f"{k}={v}" for k, v in sorted(res.fold_of_unit.items())]))
    pt.free()


if __name__ == "__main__":
    main(sys.argv[1])
