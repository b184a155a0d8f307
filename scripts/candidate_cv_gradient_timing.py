"""Timing of the gradient of the cross-validated cost over the group weights (solvers/candidates_cv_grad.py, kernels G1 and G2 of
csrc/fsnap_cvgrad.hip) next to the cross-validation it differentiates, the numpy host route and finite differences.

    python scripts/candidate_cv_gradient_timing.py [--out profiles/candidate_cv_gradient_timing.txt]

ONE run, the conventions of scripts/candidate_cv_timing.py: the driver starts one child process per shape, each under its own
``timeout -k 10``, one after the other, and stops at the first child that fails.  Shapes as there: the golden Ta rows
(15 213 x 31), synthetic 13 035 x 142 and 10^6 x 128 in 6 065 configurations, 40 groups x 3 row types; F = 5 folds; P = 32 and
128 seeded GA-style candidates.  Wall figures are medians of --reps warm synchronous calls (host timers: launches, copies and the
stream wait are inside); the kernel figures are medians of the device times between stream events of the same calls:
  g1_rhs_ms, g2_ms, g1_bilinear_ms   kernels V0 + G1 (RHS epilogue), G2, G1 (bilinear epilogue)   (events)
  grad_abi_ms      fsnap_cv_candidates_grad, the whole C call (tables, copies, the three kernels, the sums over the folds)
  gradient_ms      CandidateFits.cross_validate_gradient(method="device"): cross_validate + omega + the C call
  cv_ms            CandidateFits.cross_validate(method="device") on the same statistics
  host_ms          CandidateFits.cross_validate_gradient(method="host") (numpy from the downloaded blocks; --host-reps calls)
  fd_scaled_ms     finite differences, SCALED: the time of ONE pair of cross_validate calls x the number of active (training,
                   weighted) categories -- 2 C_active calls per candidate batch; not run in full
  gradient_over_cv = gradient_ms / cv_ms (expected, not a test: at most 3 at 10^6 x 128, P = 32)."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from candidate_cv_timing import F, candidates, median_ms, rows_of  # noqa: E402

SHAPES = {"15213x31": 240, "13035x142": 300, "1e6x128": 560}        # child time limits in seconds
WEIGHTS = {"Energy": 1.0, "Force": 0.3, "Stress": 0.01}


def child(name, reps, host_reps):
    from fitsnap_amd.config import Config
    from fitsnap_amd.parallel_tools import ParallelTools
    from fitsnap_amd.solvers import CandidateFits, solver_factory
    from fitsnap_amd.solvers import candidates_cv_grad as cg

    A, b, fs = rows_of(name)
    pt = ParallelTools()
    s = solver_factory.solver("SVD", pt, Config(pt, {"SOLVER": {"solver": "SVD"}}))
    cf = CandidateFits(s, A, b, fs_dict=fs)
    groups = sorted(set(fs["Groups"]))
    K, C = cf.K, cf.ncat
    for P in (32, 128):
        S = cf.scales_from_group_weights(candidates(groups, P, 5))
        r = cf.cross_validate_gradient(S, WEIGHTS, folds=F, by="Configs", method="device")   # prepares the composite layout
        ctx, tag = pt.hip(), cf._cv[0]
        ok = ~r.status.any(axis=1)
        omega = np.where(ok[:, None], r.omega, 0.0)
        kern = []

        def abi():
            ctx.cv_candidates_grad(tag, 0.0, S, omega, r.cv.coef)
            kern.append(ctx.cv_candidates_grad_times())

        rec = {"shape": name, "K": K, "C": C, "F": F, "P": P, "problems": P * F, "failed_candidates": int((~ok).sum()),
               "active_categories": int(np.count_nonzero((r.omega[ok] != 0).any(axis=0))) if ok.any() else 0,
               "block_bytes": F * C * (K * K + K + 3) * 8}
        rec["grad_abi_ms"] = median_ms(abi, reps)
        k = np.median(np.array(kern[1:]), axis=0)
        rec.update(g1_rhs_ms=float(k[0]), g2_ms=float(k[1]), g1_bilinear_ms=float(k[2]))
        rec["gradient_ms"] = median_ms(lambda: cf.cross_validate_gradient(S, WEIGHTS, folds=F, by="Configs", method="device"), reps)
        rec["cv_ms"] = median_ms(lambda: cf.cross_validate(S, folds=F, by="Configs", method="device"), reps)
        rec["gradient_over_cv"] = rec["gradient_ms"] / rec["cv_ms"]
        t0 = time.perf_counter()
        host = cf.cross_validate_gradient(S, WEIGHTS, folds=F, by="Configs", method="host")
        first = time.perf_counter() - t0
        rec["host_ms"] = 1e3 * first if host_reps <= 1 else median_ms(
            lambda: cf.cross_validate_gradient(S, WEIGHTS, folds=F, by="Configs", method="host"), host_reps - 1)
        up, dn = S.copy(), S.copy()
        up[:, 0] *= np.exp(1e-5)
        dn[:, 0] *= np.exp(-1e-5)

        def pair():
            cf.cross_validate(up, folds=F, by="Configs", method="device")
            cf.cross_validate(dn, folds=F, by="Configs", method="device")

        rec["fd_pair_ms"] = median_ms(pair, reps)
        rec["fd_scaled_ms"] = rec["fd_pair_ms"] * rec["active_categories"]
        rec["fd_scaled_note"] = "scaled from one pair of cross_validate calls to 2 x active categories"
        scale = np.max(np.abs(r.grad_S[ok]), axis=1, keepdims=True)
        rec["max_device_vs_host_of_largest_component"] = float(np.max(np.abs(r.grad_S[ok] - host.grad_S[ok]) / scale))
        print(json.dumps(rec), flush=True)
        assert cf._cv[0] == tag                                          # every timed call ran on the same statistics
    pt.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--shape", default=None, help="run one shape in this process (what the driver starts)")
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    args = ap.parse_args()
    if args.shape:
        child(args.shape, args.reps, args.host_reps)
        return 0
    lines = ["# scripts/candidate_cv_gradient_timing.py on one MI355X (gfx950): medians of warm calls, wall ms (kernels: device ms "
             "between stream events), one run"]
    for name, limit in SHAPES.items():
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--shape", name,
                            "--reps", str(args.reps), "--host-reps", str(args.host_reps)], stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, text=True)
        got = [l for l in r.stdout.splitlines() if l.startswith("{")]
        print("\n".join(got), flush=True)
        lines += got
        if args.out:                                                     # kept as far as the run got
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        if r.returncode != 0:                                            # a failure ends the run: nothing more is started
            print(f"{name}: exit {r.returncode}\n{r.stderr[-2000:]}", file=sys.stderr)
            return r.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
