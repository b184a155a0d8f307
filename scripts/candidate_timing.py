"""Timing of the batched candidate fits (solvers/candidates.py, kernels C1-C3 of csrc/fsnap_cand.hip) against the
single-candidate loop they replace (perform_fit + error_analysis with keep_resident).

    python scripts/candidate_timing.py                 # wall ms per candidate
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o cand -- python scripts/candidate_timing.py --kernels-only

Shapes: the golden Ta rows (15 213 x 31, its groups), synthetic 13 035 x 142 with 10 groups and 10^6 x 128 with 40 groups
(rows of 8: 1 energy, 6 force, 1 stress; a fifth of the configurations test).  Batch sizes P = 1, 8, 32, 50 of seeded
GA-style candidates (energy weight 1e-4 ... 1e4 per group, force and stress ratios 1e-3 ... 1e3).  Per shape and P: one
warm-up round, then the best of --reps rounds of (fit + frames=False errors) and of (fit + DataFrame errors), divided by
P; the loop: perform_fit + error_analysis per candidate with keep_resident, best of --reps over 8 candidates.  The row
labels are numpy arrays (the containers whose content stamps cost least, see Solver._labels_stamp) for both."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from fitsnap_amd.config import Config  # noqa: E402
from fitsnap_amd.parallel_tools import ParallelTools  # noqa: E402
from fitsnap_amd.solvers import CandidateFits, solver_factory  # noqa: E402


def candidates(groups, P, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(P):
        ew = 10.0 ** rng.uniform(-4, 4, len(groups))
        fr = 10.0 ** rng.uniform(-3, 3, len(groups))
        sr = 10.0 ** rng.uniform(-3, 3, len(groups))
        out.append({g: {"eweight": ew[i], "fweight": ew[i] * fr[i], "vweight": ew[i] * sr[i]} for i, g in enumerate(groups)})
    return out


def shapes(which):
    if "ta" in which:
        z = np.load(os.path.join(ROOT, "tests", "golden", "ta_abw.npz"))
        f = np.load(os.path.join(ROOT, "tests", "golden", "ta_reference_fits.npz"))
        fs = {"Groups": np.asarray(f["ea_groups"]).astype(str), "Testing": np.asarray(f["testing_mask"], dtype=bool),
              "Row_Type": np.array(["Energy"] * 363 + ["Force"] * 12672 + ["Stress"] * 2178)}
        yield "15213x31", np.ascontiguousarray(z["A"]), np.ascontiguousarray(z["b"]), np.ascontiguousarray(z["w"]), fs
    r = np.random.default_rng(1)
    for name, m, K, ng in (("13035x142", 13_035, 142, 10), ("1e6x128", 1_000_000, 128, 40)):
        if name not in which:
            continue
        m8 = m // 8 * 8
        A = r.standard_normal((m8, K)) * np.exp(0.5 * r.standard_normal(K))
        b = A @ r.standard_normal(K) + 0.05 * r.standard_normal(m8)
        g = np.repeat(r.integers(0, ng, m8 // 8), 8)
        test = np.repeat(r.random(m8 // 8) < 0.2, 8)
        fs = {"Groups": np.char.add("g", np.char.zfill(g.astype(str), 2)), "Testing": test,
              "Row_Type": np.tile(np.array(["Energy"] + ["Force"] * 6 + ["Stress"]), m8 // 8)}
        yield name, A, b, 0.5 + r.random(m8), fs


def best(f, reps):
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        t.append(time.perf_counter() - t0)
    return min(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="ta,13035x142,1e6x128")
    ap.add_argument("--kernels-only", action="store_true", help="P = 16 fit + errors rounds only (for a kernel trace)")
    args = ap.parse_args()
    for name, A, b, w0, fs in shapes(args.shapes):
        pt = ParallelTools()
        s = solver_factory.solver("SVD", pt, Config(pt, {"SOLVER": {"solver": "SVD"}}))
        t0 = time.perf_counter()
        cf = CandidateFits(s, A, b, w0=w0, fs_dict=fs)
        cf.fit(np.ones((1, cf.ncat)))                       # layout + per-category statistics (once per rows)
        setup = time.perf_counter() - t0
        groups = sorted(set(fs["Groups"]))
        if args.kernels_only:
            S = cf.scales_from_group_weights(candidates(groups, 16, 5))
            for _ in range(args.reps):
                cf.errors(cf.fit(S), S, frames=False)
            pt.free()
            continue
        for P in (1, 8, 32, 50):
            S = cf.scales_from_group_weights(candidates(groups, P, 5))
            cf.errors(cf.fit(S), S, frames=False)
            lean = best(lambda: cf.errors(cf.fit(S), S, frames=False), args.reps)
            frames = best(lambda: cf.errors(cf.fit(S), S), args.reps)
            paths = sorted({i["path"] for i in cf.info})
            print(json.dumps({"shape": name, "P": P, "ms_per_candidate_lean": 1e3 * lean / P,
                              "ms_per_candidate_frames": 1e3 * frames / P, "paths": paths, "setup_s": setup}), flush=True)
        # the loop the batch replaces: one perform_fit + error_analysis per candidate on resident rows
        s2 = solver_factory.solver("SVD", pt, Config(pt, {"SOLVER": {"solver": "SVD"}}))
        s2.keep_resident = True
        S = cf.scales_from_group_weights(candidates(groups, 8, 6))
        t = ~np.asarray(fs["Testing"], dtype=bool)
        W = [cf.row_weights(S[p]) for p in range(8)]

        def loop():
            for wf in W:
                s2.perform_fit(A, b, wf[t], fs_dict=fs)
                s2.error_analysis(A, b, wf, fs)

        loop()
        print(json.dumps({"shape": name, "loop_ms_per_candidate": 1e3 * best(loop, args.reps) / 8}), flush=True)
        pt.free()


if __name__ == "__main__":
    main()
