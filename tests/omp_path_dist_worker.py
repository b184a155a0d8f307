"""Worker of tests/test_gpu_omp_path.py: one rank of a sparse-selection-path run (peer-to-peer transport; the ranks may share
one GPU), launched with RANK / WORLD_SIZE / LOCAL_RANK / FSNAP_COMM_FILE / FSNAP_DIST_TRANSPORT in the environment.  Row i lives
on rank i % world, so every configuration spans the ranks; every rank fits OMP on its shared rows and calls omp_path().  Writes
what the rank got to <outdir>/omp_rank<r>.npz."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SIZES = [12 + (7 * c) % 40 for c in range(30)]
TERMS = 12
SECTION = {"terms": TERMS, "criterion": "ols", "forced": "4"}


def rows():
    from loco_cases import config_rows

    return config_rows(11, 31, SIZES, testing_frac=0.1)


def path_of(solver):
    return solver.omp_path(20, levels=[1, 5, TERMS, 20], criterion="ols", forced=(4,), folds=4, seed=3, method="device")


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
    s = solver_factory.solver("OMP", pt, Config(pt, {"SOLVER": {"solver": "OMP"}, "OMP": dict(SECTION)}))
    s.perform_fit()
    res = path_of(s)
    np.savez(os.path.join(outdir, f"omp_rank{rank}.npz"), order=res.order, fold_orders=res.fold_orders, levels=res.levels,
             fits=res.fits, train_sse=res.train_sse, table=res.table.to_numpy(dtype=float),
             index=np.array([str(x) for x in res.table.index]), cv_error=res.cv_error, cv_se=res.cv_se, best=res.best,
             sparsest=res.sparsest, frequency=res.frequency, solver_order=s.order,
             folds=np.array([f"{k}={v}" for k, v in sorted(res.fold_of_unit.items())]))
    pt.free()


if __name__ == "__main__":
    main(sys.argv[1])
