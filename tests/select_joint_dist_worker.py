"""Worker of tests/test_gpu_select_joint.py: one rank of a two-rank joint unit selection (peer-to-peer transport; both ranks may
share one GPU), launched with RANK / WORLD_SIZE / LOCAL_RANK / FSNAP_COMM_FILE / FSNAP_DIST_TRANSPORT in the environment.
Every rank owns the pool configurations c with c % world == rank; the prior covariance and the noise variance are set on
rank 0 only.  The target is the pool itself (every rank's share of its Gram is summed).  Writes the rank's row ids and, per
criterion, the picked configurations, scores, dims, the covariance and the one-shot scores to <outdir>/joint_rank<r>.npz."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

BATCH = 8


def pool():
    import select_cases as sc

    return sc.clustered(21, 31, n_pool=90, size_hi=200)


def main(outdir):
    from fitsnap_amd.config import Config
    from fitsnap_amd.parallel_tools import ParallelTools
    from fitsnap_amd.solvers import solver_factory

    pt = ParallelTools(comm="rccl")
    rank, world = pt._rank, pt._size
    p = pool()
    mine = np.flatnonzero(p["cat"] % world == rank)
    s = solver_factory.solver("ANL", pt, Config(pt, {"SOLVER": {"solver": "ANL"}}))
    if rank == 0:
        s.cov, s.sigmahat = p["C0"], p["tau"]
    A = np.ascontiguousarray(p["A"][mine])
    labels = [f"cfg{c}" for c in p["cat"][mine]]
    out = {"rows": mine}
    for crit in ("gain", "reduction"):
        res = s.select_units(BATCH, a=A, w=p["w"][mine], categories=labels, criterion=crit, row_scale=p["s"][mine])
        out.update({f"{crit}_picked": np.array([int(k[3:]) for k in res.keys]), f"{crit}_scores": res.scores,
                    f"{crit}_dims": np.array(res.dims), f"{crit}_cov": res.cov, f"{crit}_initial": res.initial_scores,
                    f"{crit}_keys": np.array([int(k[3:]) for k in res.all_keys])})
    np.savez(os.path.join(outdir, f"joint_rank{rank}.npz"), **out)
    pt.free()


if __name__ == "__main__":
    main(sys.argv[1])
