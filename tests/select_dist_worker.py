"""Worker of tests/test_gpu_select.py: one rank of a two-rank greedy batch selection (peer-to-peer transport; both ranks may
share one GPU), launched with RANK / WORLD_SIZE / LOCAL_RANK / FSNAP_COMM_FILE / FSNAP_DIST_TRANSPORT in the environment.
Every rank owns the pool configurations c with c % world == rank (every unit lives on one rank); the prior covariance is
set on rank 0 only and reaches the other rank by broadcast, like the noise variance.  Writes the rank's row ids, the picked
configurations, scores, ranks, factors, the covariance and its rows' variances to <outdir>/select_rank<r>.npz."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

BATCH = 10


def pool():
    import select_cases as sc

    return sc.clustered(21, 31, n_pool=90, size_hi=200)


def main(outdir):
    from fitsnap_amd.config import Config
    from fitsnap_amd.parallel_tools import ParallelTools
    from fitsnap_amd.solvers import select, solver_factory

    pt = ParallelTools(comm="rccl")
    rank, world = pt._rank, pt._size
    p = pool()
    mine = np.flatnonzero(p["cat"] % world == rank)
    s = solver_factory.solver("ANL", pt, Config(pt, {"SOLVER": {"solver": "ANL"}}))
    if rank == 0:
        s.cov, s.sigmahat = p["C0"], p["tau"]
    res = select.select_batch(s, BATCH, a=np.ascontiguousarray(p["A"][mine]), w=p["w"][mine],
                              categories=[f"cfg{c}" for c in p["cat"][mine]], row_scale=p["s"][mine], keep_factors=True)
    out = {"rows": mine, "picked": np.array([int(k[3:]) for k in res.keys]), "scores": res.scores, "ranks": np.array(res.ranks),
           "cov": res.cov, "var": res.var}
    out.update({f"V{t}": V for t, V in enumerate(s._select_factors)})
    np.savez(os.path.join(outdir, f"select_rank{rank}.npz"), **out)
    pt.free()


if __name__ == "__main__":
    main(sys.argv[1])
