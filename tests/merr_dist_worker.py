"""Worker of tests/test_gpu_merr.py: one rank of a two-rank MERR fit (peer-to-peer transport; both ranks may share one
GPU), launched with RANK / WORLD_SIZE / LOCAL_RANK / FSNAP_COMM_FILE / FSNAP_DIST_TRANSPORT in the environment.  Every rank
owns the blocks of 43 rows i with i % world == rank of the row subset of tests/golden/ta_merr_reference.npz, fits with
MERR (iid, additive; numpy seeded with the rank, so the ranks draw different starts) and writes its start, result and the
log-posterior / gradient at a fixed vector to <outdir>/merr_rank<r>.npz."""
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
    ref = np.load(os.path.join(ROOT, "tests", "golden", "ta_merr_reference.npz"))
    z = np.load(os.path.join(ROOT, "tests", "golden", "ta_abw.npz"))
    st = int(ref["row_stride"])
    A, b, w = z["A"][::st], z["b"][::st], z["w"][::st]
    mine = (np.arange(len(b)) // 43 % world) == rank
    cfg = Config(pt, {"SOLVER": {"solver": "MERR", "merr_method": "iid", "merr_mult": 0, "merr_cfs": "all"}})
    s = solver_factory.solver("MERR", pt, cfg)
    s.save_files = False
    np.random.seed(rank)          # each rank draws a start of its own: the class must take rank 0's
    s.perform_fit(np.ascontiguousarray(A[mine]), np.ascontiguousarray(b[mine]), np.ascontiguousarray(w[mine]), trainall=True)
    x = np.array(ref["iid_add_x"])
    f, grad = s.objective(x)
    np.savez(os.path.join(outdir, f"merr_rank{rank}.npz"), fit=s.fit, f=np.float64(f), grad=grad, x=x,
             params_ini=s.params_ini, params=s.params, evaluations=np.int64(s.evaluations))
    pt.free()


if __name__ == "__main__":
    main(sys.argv[1])
