"""Worker of tests/test_gpu_uq.py: one rank of a two-rank predictive-variance pass (peer-to-peer transport; both ranks may
share one GPU), launched with RANK / WORLD_SIZE / LOCAL_RANK / FSNAP_COMM_FILE / FSNAP_DIST_TRANSPORT in the environment.
Every rank owns the blocks of 43 Ta rows i with i % world == rank as its shared rows; the ANL posterior of
tests/golden/ta_stdev_reference.npz is set on rank 0 only (where a fit lives) and reaches the other rank by broadcast.
Writes the rank's row ids, stdevs of three methods and predictions to <outdir>/uq_rank<r>.npz."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(outdir):
    from fitsnap_amd.config import Config
    from fitsnap_amd.parallel_tools import ParallelTools
    from fitsnap_amd.solvers import solver_factory

    pt = ParallelTools(comm="rccl")
    rank, world = pt._rank, pt._size
    z = np.load(os.path.join(ROOT, "tests", "golden", "ta_abw.npz"))
    g = np.load(os.path.join(ROOT, "tests", "golden", "ta_stdev_reference.npz"))
    A, b, w = z["A"], z["b"], z["w"]
    mine = np.flatnonzero((np.arange(len(b)) // 43 % world) == rank)
    pt.create_shared_array("a", len(mine), A.shape[1])
    pt.create_shared_array("b", len(mine))
    pt.create_shared_array("w", len(mine))
    pt.shared_arrays["a"].array[:] = A[mine]
    pt.shared_arrays["b"].array[:] = b[mine]
    pt.shared_arrays["w"].array[:] = w[mine]
    s = solver_factory.solver("ANL", pt, Config(pt, {"SOLVER": {"solver": "ANL"}}))
    if rank == 0:
        s.cov, s.fit, s.fit_sam = g["cov"], g["fit"], g["fit_sam"]
    out = {"rows": mine}
    for meth in ("sam", "chol", "fullcov"):
        out[f"stdev_{meth}"] = s._compute_stdev(method=meth)
    out["preds"] = s.prediction_variance()["preds"]
    np.savez(os.path.join(outdir, f"uq_rank{rank}.npz"), **out)
    pt.free()


if __name__ == "__main__":
    main(sys.argv[1])
