"""Worker of tests/test_gpu_candidate_cvgrad.py: one rank of a two-rank gradient of the cross-validated cost (peer-to-peer
transport; both ranks may share one GPU), launched with RANK / WORLD_SIZE / LOCAL_RANK / FSNAP_COMM_FILE /
FSNAP_DIST_TRANSPORT in the environment.  The rows are dealt as tests/candidate_cv_dist_worker.py deals them (blocks of 43 Ta
rows, units of 7: units straddle the ranks); the rank evaluates the seeded GA-style candidates of tests/candidate_cv_cases.py
with RIDGE, takes two descent steps from the first three and writes everything to <outdir>/cvgrad_rank<r>.npz."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main(outdir):
    import candidate_cv_cases as cc
    import candidate_cvgrad_cases as gc
    from fitsnap_amd.config import Config
    from fitsnap_amd.parallel_tools import ParallelTools
    from fitsnap_amd.solvers import CandidateFits, solver_factory

    pt = ParallelTools(comm="rccl")
    rank, world = pt._rank, pt._size
    z = np.load(os.path.join(ROOT, "tests", "golden", "ta_abw.npz"))
    fits = dict(np.load(os.path.join(ROOT, "tests", "golden", "ta_reference_fits.npz")))
    A, b = z["A"], z["b"]
    fs_all = cc.ta_labels(fits)
    mine = (np.arange(len(b)) // 43 % world) == rank
    fs = {k: [x for x, keep in zip(v, mine) if keep] for k, v in fs_all.items()}
    cfg = Config(pt, {"SOLVER": {"solver": "RIDGE"}, "RIDGE": {"alpha": cc.TA_ALPHAS["RIDGE"]}})
    s = solver_factory.solver("RIDGE", pt, cfg)
    cf = CandidateFits(s, np.ascontiguousarray(A[mine]), np.ascontiguousarray(b[mine]), fs_dict=fs)
    S = cf.scales_from_group_weights(cc.ta_candidates(sorted(set(fs_all["Groups"])), cc.TA_P, seed=11))
    r = cf.cross_validate_gradient(S, gc.TA_WEIGHTS, folds=cc.TA_F, by="Configs")
    dS, hist, _ = cf.descend_weights(S[:3], gc.TA_WEIGHTS, steps=2, folds=cc.TA_F, by="Configs")
    np.savez(os.path.join(outdir, f"cvgrad_rank{rank}.npz"), cost=r.cost, grad_S=r.grad_S, grad_log=r.grad_log,
             grad_log_alpha=r.grad_log_alpha, omega=r.omega, status=r.status, coef=r.cv.coef, descent_S=dS, descent_history=hist)
    pt.free()


if __name__ == "__main__":
    main(sys.argv[1])
