"""Worker of tests/test_gpu_loco.py: one rank of a two-rank leave-one-configuration-out run (peer-to-peer transport; both
ranks may share one GPU), launched with RANK / WORLD_SIZE / LOCAL_RANK / FSNAP_COMM_FILE / FSNAP_DIST_TRANSPORT in the
environment.  The configurations are dealt round-robin (configuration c on rank c % world, as the calculator deals them);
every rank fits RIDGE on its shared rows and calls loco_errors().  Writes the rank's row ids, LOO predictions, the M and
beta the ranks used and (rank 0) the error table to <outdir>/loco_rank<r>.npz."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main(outdir):
    from loco_cases import config_rows

    from fitsnap_amd.config import Config
    from fitsnap_amd.parallel_tools import ParallelTools
    from fitsnap_amd.solvers import loco, solver_factory

    pt = ParallelTools(comm="rccl")
    rank, world = pt._rank, pt._size
    sizes = [12 + (7 * c) % 90 for c in range(40)]
    A, b, w, labels = config_rows(5, 31, sizes, testing_frac=0.1)
    cfg = np.repeat(np.arange(len(sizes)), sizes)
    mine = np.flatnonzero(cfg % world == rank)
    pt.create_shared_array("a", len(mine), A.shape[1])
    pt.create_shared_array("b", len(mine))
    pt.create_shared_array("w", len(mine))
    pt.shared_arrays["a"].array[:] = A[mine]
    pt.shared_arrays["b"].array[:] = b[mine]
    pt.shared_arrays["w"].array[:] = w[mine]
    local = {k: [v[i] for i in mine] for k, v in labels.items()}
    pt.fitsnap_dict = dict(local)
    pt.local_lists = dict(local)
    s = solver_factory.solver("RIDGE", pt, Config(pt, {"SOLVER": {"solver": "RIDGE"}, "RIDGE": {"alpha": 1e-6}}))
    s.perform_fit()
    res = s.loco_errors()
    M = loco.smoother_factor(s)[1] if rank == 0 else None
    M = pt.bcast_object(M, src=0)
    beta = s._uq_inputs()[1]
    out = {"rows": mine, "preds": res.preds, "M": M, "beta": beta}
    if rank == 0:
        out["errors"] = res.errors.to_numpy(dtype=float)
        out["index"] = np.array([str(x) for x in res.errors.index])
        out["unit_sse"] = res.units["w_sse"].to_numpy()
        out["unit_names"] = res.units["Configs"].to_numpy().astype(str)
    np.savez(os.path.join(outdir, f"loco_rank{rank}.npz"), **out)
    pt.free()


if __name__ == "__main__":
    main(sys.argv[1])
