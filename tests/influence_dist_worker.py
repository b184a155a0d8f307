"""Worker of tests/test_gpu_influence.py: one rank of a two-rank influence run (peer-to-peer transport; both ranks may share
one GPU), launched with RANK / WORLD_SIZE / LOCAL_RANK / FSNAP_COMM_FILE / FSNAP_DIST_TRANSPORT in the environment.  The
configurations are dealt round-robin (configuration c on rank c % world, as the calculator deals them); every rank fits RIDGE
on its shared rows and calls influence(), then once more with one configuration relabelled so that it has rows on both ranks,
which must raise.  Writes the pooled unit names and Cook's distances and (rank 0) the covariances and the table of standard
errors to <outdir>/influence_rank<r>.npz."""
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
    res = s.influence(kinds=("cr0", "cr1", "jack"), noise=0.01, want_dfbeta=True)
    own = sum(1 for c in range(len(sizes)) if c % world == rank)
    assert res.dfbeta.shape == (own, A.shape[1]) and len(res.units) == len(sizes)
    out = {"unit_names": res.units["Configs"].to_numpy().astype(str), "cook": res.units["cook"].to_numpy(dtype=float)}
    if rank == 0:
        for k, v in res.cov.items():
            out["cov_" + k] = v
        out["stderr"] = res.stderr.to_numpy(dtype=float)
        out["stderr_columns"] = np.array(list(res.stderr.columns))
    else:
        assert res.cov is None and res.stderr is None
    # configurations 0 (rank 0) and 1 (rank 1) under one label: the unit has rows on both ranks
    split = dict(local)
    split["Configs"] = ["cfg0" if c == "cfg1" else c for c in local["Configs"]]
    pt.local_lists = split
    try:
        s.influence()
        out["split"] = "accepted"
    except ValueError as e:
        out["split"] = "refused" if "influence: unit 'cfg0' has rows on ranks 0 and 1" in str(e) else str(e)
    np.savez(os.path.join(outdir, f"influence_rank{rank}.npz"), **out)
    pt.free()


if __name__ == "__main__":
    main(sys.argv[1])
