"""Worker of tests/test_gpu_candidates.py: one rank of a two-rank batch of candidate fits (peer-to-peer transport; both ranks
may share one GPU), launched with RANK / WORLD_SIZE / LOCAL_RANK / FSNAP_COMM_FILE / FSNAP_DIST_TRANSPORT in the environment.
Every rank owns the blocks of 43 Ta rows i with i % world == rank, fits the seeded GA-style candidates of
tests/test_gpu_candidates.py with SVD and writes the coefficients, ranks and (rank 0) the error tables to
<outdir>/cand_rank<r>.npz."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main(outdir):
    from fitsnap_amd.config import Config
    from fitsnap_amd.parallel_tools import ParallelTools
    from fitsnap_amd.solvers import CandidateFits, solver_factory
    from test_gpu_candidates import ROW_TYPE, ga_candidates

    pt = ParallelTools(comm="rccl")
    rank, world = pt._rank, pt._size
    z = np.load(os.path.join(ROOT, "tests", "golden", "ta_abw.npz"))
    f = np.load(os.path.join(ROOT, "tests", "golden", "ta_reference_fits.npz"))
    A, b, w = z["A"], z["b"], z["w"]
    mine = (np.arange(len(b)) // 43 % world) == rank
    groups = [str(g) for g in f["ea_groups"]]
    fs = {"Groups": [g for g, k in zip(groups, mine) if k], "Testing": f["testing_mask"][mine].tolist(),
          "Row_Type": [r for r, k in zip(ROW_TYPE, mine) if k]}
    cfg = Config(pt, {"SOLVER": {"solver": "SVD"}})
    s = solver_factory.solver("SVD", pt, cfg)
    cf = CandidateFits(s, np.ascontiguousarray(A[mine]), np.ascontiguousarray(b[mine]), w0=np.ascontiguousarray(w[mine]),
                       fs_dict=fs)
    S = cf.scales_from_group_weights(ga_candidates(sorted(set(groups)), 24, seed=7))
    betas = cf.fit(S)
    tables = cf.errors(betas, S, frames=False)
    out = {"betas": betas, "ranks": np.array([i["rank"] for i in cf.info]), "ncat": np.int64(cf.ncat)}
    if rank == 0:
        out["grouped"] = np.array([t[0] for t in tables])
        out["allrows"] = np.array([t[1] for t in tables])
    else:
        out["none"] = np.int64(tables is None)
    np.savez(os.path.join(outdir, f"cand_rank{rank}.npz"), **out)
    pt.free()


if __name__ == "__main__":
    main(sys.argv[1])
