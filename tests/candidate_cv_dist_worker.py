"""Worker of tests/test_gpu_candidate_cv.py: one rank of a two-rank cross-validation of weight candidates (peer-to-peer
transport; both ranks may share one GPU), launched with RANK / WORLD_SIZE / LOCAL_RANK / FSNAP_COMM_FILE /
FSNAP_DIST_TRANSPORT in the environment.  Every rank owns the blocks of 43 Ta rows i with i // 43 % world == rank while the
units are the blocks of 7 rows, so units straddle the ranks; it cross-validates the seeded GA-style candidates of
tests/candidate_cv_cases.py with SVD and writes coefficients, pooled sums, tables, costs and folds to
<outdir>/cv_rank<r>.npz."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main(outdir):
    import candidate_cv_cases as cc
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
    here = set(fs["Configs"])
    elsewhere = {u for u, keep in zip(fs_all["Configs"], mine) if not keep}
    cfg = Config(pt, {"SOLVER": {"solver": "SVD"}})
    s = solver_factory.solver("SVD", pt, cfg)
    cf = CandidateFits(s, np.ascontiguousarray(A[mine]), np.ascontiguousarray(b[mine]), fs_dict=fs)
    S = cf.scales_from_group_weights(cc.ta_candidates(sorted(set(fs_all["Groups"])), cc.TA_P, seed=11))
    cv = cf.cross_validate(S, folds=cc.TA_F, by="Configs")
    units = sorted(cv.fold_of_unit)
    np.savez(os.path.join(outdir, f"cv_rank{rank}.npz"), coef=cv.coef, status=cv.status, sums=cv.sums,
             tables=cv.tables(frames=False)[1], cost=cv.cost({"Energy": 1.0, "Force": 0.3, "Stress": 0.01}),
             fold_units=np.array(units), fold_ids=np.array([cv.fold_of_unit[u] for u in units]),
             split_units=np.int64(len(here & elsewhere)))
    pt.free()


if __name__ == "__main__":
    main(sys.argv[1])
