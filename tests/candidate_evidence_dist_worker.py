"""Worker of tests/test_gpu_candidate_evidence.py: one rank of a two-rank evidence of weight candidates (peer-to-peer transport;
both ranks may share one GPU), launched with RANK / WORLD_SIZE / LOCAL_RANK / FSNAP_COMM_FILE / FSNAP_DIST_TRANSPORT in the
environment.  The rows are dealt as tests/candidate_cvgrad_dist_worker.py deals them (blocks of 43 Ta rows); the rank evaluates
the candidates of ``candidate_evidence_cases.ta_case`` with RIDGE, takes two ascent steps from the first three and writes
everything to <outdir>/evidence_rank<r>.npz."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main(outdir):
    import candidate_cv_cases as cc
    import candidate_evidence_cases as ec
    from fitsnap_amd.config import Config
    from fitsnap_amd.parallel_tools import ParallelTools
    from fitsnap_amd.solvers import CandidateFits, solver_factory
    from fitsnap_amd.solvers import candidates_evidence as ce

    pt = ParallelTools(comm="rccl")
    rank, world = pt._rank, pt._size
    fits = dict(np.load(os.path.join(ROOT, "tests", "golden", "ta_reference_fits.npz")))
    A, b, _, _, keys, S, _ = ec.ta_case()
    fs_all = cc.ta_labels(fits)
    mine = (np.arange(len(b)) // 43 % world) == rank
    fs = {k: [x for x, keep in zip(v, mine) if keep] for k, v in fs_all.items()}
    cfg = Config(pt, {"SOLVER": {"solver": "RIDGE"}, "RIDGE": {"alpha": cc.TA_ALPHAS["RIDGE"]}})
    s = solver_factory.solver("RIDGE", pt, cfg)
    cf = CandidateFits(s, np.ascontiguousarray(A[mine]), np.ascontiguousarray(b[mine]), fs_dict=fs)
    assert cf.keys == keys
    ev = cf.evidence(S)
    aS, _, hist, conv = cf.maximise_evidence(S[:3], steps=2)
    np.savez(os.path.join(outdir, f"evidence_rank{rank}.npz"), active=ev.active, ascent_S=aS, ascent_history=hist, ascent_converged=conv,
             **{f: getattr(ev, f) for f in ce.FIELDS})
    pt.free()


if __name__ == "__main__":
    main(sys.argv[1])
