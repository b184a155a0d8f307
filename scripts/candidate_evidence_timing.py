"""Timing of the marginal likelihood of group-weight candidates (solvers/candidates_evidence.py, kernels E1-E3 of
csrc/fsnap_evidence.hip) next to the numpy host route and to one batched fit with lean error tables of the same candidates.

    python scripts/candidate_evidence_timing.py [--out profiles/candidate_evidence_timing.txt]

ONE run, the conventions of scripts/candidate_cv_gradient_timing.py: the driver starts one child process per shape, each under
its own ``timeout -k 10``, one after the other, and stops at the first child that fails.  Shapes as there: the golden Ta rows
(15 213 x 31), synthetic 13 035 x 142 and 10^6 x 128 in 6 065 configurations, 40 groups x 3 row types; P = 32 and 128 seeded
GA-style candidates.  Wall figures are medians of --reps warm synchronous calls (host timers: launches, copies and the stream
wait are inside); the kernel figures are medians of the device times between stream events of the same calls:
  e1_ms, e2_e3_ms  kernel E1 (factor, log-determinant, in-place inverse, tables), kernels E2 + E3 (the MFMA sweep)   (events)
  abi_ms           fsnap_candidates_evidence, the whole C call (masked scales, the three kernels, copies)
  evidence_ms      CandidateFits.evidence(method="device"): the C call + the float64 assembly
  host_ms          CandidateFits.evidence(method="host") (numpy from the downloaded blocks; --host-reps calls)
  fit_errors_ms    one CandidateFits.fit(S) + errors(betas, S, frames=False) of the same batch
  evidence_over_fit_errors = evidence_ms / fit_errors_ms (expected, not a test: at most 2 at P = 32)."""
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

from candidate_cv_timing import candidates, median_ms, rows_of  # noqa: E402

SHAPES = {"15213x31": 240, "13035x142": 300, "1e6x128": 560}        # child time limits in seconds


def child(name, reps, host_reps):
    from fitsnap_amd.config import Config
    from fitsnap_amd.parallel_tools import ParallelTools
    from fitsnap_amd.solvers import CandidateFits, solver_factory
    from fitsnap_amd.solvers import candidates_evidence as ce

    A, b, fs = rows_of(name)
    pt = ParallelTools()
    s = solver_factory.solver("SVD", pt, Config(pt, {"SOLVER": {"solver": "SVD"}}))
    cf = CandidateFits(s, A, b, fs_dict=fs)
    groups = sorted(set(fs["Groups"]))
    K, C = cf.K, cf.ncat
    for P in (32, 128):
        S = cf.scales_from_group_weights(candidates(groups, P, 5))
        ev = cf.evidence(S, method="device")                             # prepares the layout and its statistics
        ctx, tag = pt.hip(), cf._layout
        n, _, training = ce.evidence_constants(cf)
        active = ce.active_mask(S, training, n)
        kern = []

        def abi():
            ctx.candidates_evidence(tag, 0.0, S, active, K)
            kern.append(ctx.candidates_evidence_times())

        rec = {"shape": name, "K": K, "C": C, "P": P, "failed_candidates": int(np.count_nonzero(ev.status)),
               "active_categories": int(np.count_nonzero(ev.active.any(axis=0))), "block_bytes": C * (K * K + K + 3) * 8}
        rec["abi_ms"] = median_ms(abi, reps)
        k = np.median(np.array(kern[1:]), axis=0)
        rec.update(e1_ms=float(k[0]), e2_e3_ms=float(k[1]))
        rec["evidence_ms"] = median_ms(lambda: cf.evidence(S, method="device"), reps)
        t0 = time.perf_counter()
        host = cf.evidence(S, method="host")
        first = time.perf_counter() - t0
        rec["host_ms"] = 1e3 * first if host_reps <= 1 else median_ms(lambda: cf.evidence(S, method="host"), host_reps - 1)

        def fit_errors():
            cf.errors(cf.fit(S), S, frames=False)

        rec["fit_errors_ms"] = median_ms(fit_errors, reps)
        rec["evidence_over_fit_errors"] = rec["evidence_ms"] / rec["fit_errors_ms"]
        ok = (ev.status == 0) & (host.status == 0)
        N = np.where(ev.active, ce.evidence_constants(cf)[0][None, :], 0.0).sum(axis=1)
        rec["max_device_vs_host_L_per_row"] = float(np.max(np.abs(ev.log_evidence - host.log_evidence)[ok] / N[ok])) if ok.any() else None
        print(json.dumps(rec), flush=True)
        assert cf._layout == tag                                         # every timed call ran on the same statistics
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
    lines = ["# scripts/candidate_evidence_timing.py on one MI355X (gfx950): medians of warm calls, wall ms (kernels: device ms "
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
