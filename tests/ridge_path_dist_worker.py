"""Worker of tests/test_gpu_ridge_path.py: one rank of a two-rank ridge-path run (peer-to-peer transport; both ranks may
share one GPU), launched with RANK / WORLD_SIZE / LOCAL_RANK / FSNAP_COMM_FILE / FSNAP_DIST_TRANSPORT in the environment.
The configurations are dealt round-robin (configuration c on rank c % world); every rank fits RIDGE on its shared rows and
calls ridge_path().  Writes the rank's row ids, the Q x rows predictions, the statistics the ranks used, the table, its index,
``best`` and the unit frame's (alpha|unit) names to <outdir>/path_rank<r>.npz."""
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
    from fitsnap_amd.solvers import solver_factory

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
    alphas = np.array([0.0, 1e-8, 1e-4, 1e-2, 1.0])
    res = s.ridge_path(alphas, want_preds=True)
    stats = pt.bcast_object(None if rank != 0 else (np.asarray(s.last_statistics[0]), np.asarray(s.last_statistics[1])), src=0)
    out = {"rows": mine, "preds": res.preds, "G": stats[0], "c": stats[1], "alphas": alphas,
           "table": res.table.to_numpy(dtype=float), "index": np.array([str(x) for x in res.table.index]),
           "best": -1 if res.best is None else res.best,
           "unit_names": np.array([f"{a:g}|{u}" for a, u in zip(res.units["alpha"], res.units["Configs"])])}
    np.savez(os.path.join(outdir, f"path_rank{rank}.npz"), **out)
    pt.free()


if __name__ == "__main__":
    main(sys.argv[1])
