"""Worker of tests/test_gpu_robust.py: one rank of a two-rank robust fit (peer-to-peer transport; both ranks may share one
GPU), launched with RANK / WORLD_SIZE / LOCAL_RANK / FSNAP_COMM_FILE / FSNAP_DIST_TRANSPORT in the environment.  Two deals
of the rows of the standard 3000 x 17 case: "split" (row i on rank i % world) and "empty" (every row on rank 0, rank 1 holds
none).  Per deal: the scales of one selection at a beta every rank derives from the same seed, then ``Solver.robust_fit``
with 12 fixed iterations.  Writes <outdir>/robust_rank<r>.npz."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main(outdir):
    import robust_cases as rc

    from fitsnap_amd.config import Config
    from fitsnap_amd.parallel_tools import ParallelTools
    from fitsnap_amd.solvers import solver_factory

    pt = ParallelTools(comm="rccl")
    rank, world = pt._rank, pt._size
    cs = rc.case(3000, 17)
    beta = rc.probe_beta(cs)
    s = solver_factory.solver("ROBUST", pt, Config(pt, {"SOLVER": {"solver": "ROBUST"}}))
    out = {}
    for deal in ("split", "empty"):
        rows = np.arange(cs.m)
        mine = rows[rows % world == rank] if deal == "split" else (rows if rank == 0 else rows[:0])
        ctx = pt.hip()
        if len(mine):
            ctx.upload_rows(cs.A[mine], cs.b[mine])
            ctx.set_weights(cs.w[mine], cs.mask[mine].astype(np.uint8))
        elif ctx.m > 0:
            ctx.drop_rows()
        ctx.robust_begin(cs.cat[mine] if len(mine) else None, 3)
        try:
            ctx.robust_residuals(beta)
            scale, count = ctx.robust_scale()
        finally:
            ctx.robust_end()
        out[deal + "_scale"], out[deal + "_count"] = scale, count
        labels = {"Testing": (~cs.mask[mine]).tolist(), "Row_Type": cs.row_type[mine].tolist()}
        res = s.robust_fit(loss="huber", alpha=rc.ALPHA, max_iter=rc.FIXED_ITERS, tol=0.0, a=cs.A[mine], b=cs.b[mine],
                           w=cs.w[mine][cs.mask[mine]], fs_dict=labels)
        out[deal + "_fit"], out[deal + "_scales"], out[deal + "_tables"] = res.fit, res.scales, res.tables
        out[deal + "_omega"], out[deal + "_rows"] = res.omega(), mine
    np.savez(os.path.join(outdir, f"robust_rank{rank}.npz"), **out)
    pt.free()


if __name__ == "__main__":
    main(sys.argv[1])
