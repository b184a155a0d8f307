"""Timing of the MERR log-posterior pass (fsnap_merr_eval, kernel M1 / M2 + M3) and of whole MERR fits.

    python scripts/merr_timing.py                 # evaluations and fits, wall times
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o merr -- python scripts/merr_timing.py --evals-only
    python scripts/merr_timing.py --kernel-trace <dir>/merr_kernel_trace.csv   # kernel times -> share of 8 TB/s

Shapes: 10^6 x 128 (synthetic), 13 035 x 142 (the PACE width, synthetic) and 15 213 x 31 (the golden Ta rows).  One
evaluation moves 8K + 17 bytes per row (the row, b, w, the mask byte); the share of HBM bandwidth is reported against
8 TB/s.  fsnap_merr_eval synchronises, so its wall time includes the 2K-double upload and the (2K + 1)-double download;
the kernel time comes from the trace of an --evals-only run with the same --reps: per shape, the median over the timed
calls of the MERR kernel(s) plus their fold.  Fits: a warm-up fit of the shape, then the timed fit of the same arrays
in the same process (both seeded with np.random.seed(0))."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from fitsnap_amd import _capi  # noqa: E402
from fitsnap_amd.config import Config  # noqa: E402
from fitsnap_amd.parallel_tools import ParallelTools  # noqa: E402
from fitsnap_amd.solvers import solver_factory  # noqa: E402

HBM = 8.0e12


def shapes():
    r = np.random.default_rng(1)
    for name, m, K in (("1e6x128", 1_000_000, 128), ("13035x142", 13_035, 142)):
        A = r.standard_normal((m, K)) * np.exp(0.5 * r.standard_normal(K))
        b = A @ r.standard_normal(K) + 0.05 * r.standard_normal(m) * (1.0 + np.abs(A[:, 0]))
        yield name, A, b, 0.5 + r.random(m)
    z = np.load(os.path.join(ROOT, "tests", "golden", "ta_abw.npz"))
    yield "15213x31", np.ascontiguousarray(z["A"]), np.ascontiguousarray(z["b"]), np.ascontiguousarray(z["w"])


def kernel_shares(path, reps):
    """Per shape (in the order of shapes()): median kernel time of the timed calls of an --evals-only run."""
    import csv

    rows = [r for r in csv.DictReader(open(path)) if "fsnap_merr" in r["Kernel_Name"] or "fsnap_colsum" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    calls, cur = [], []
    for r in rows:                        # a call = its MERR kernel(s) up to and including the fold
        cur.append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-9)
        if "fsnap_colsum" in r["Kernel_Name"]:
            calls.append(sum(cur))
            cur = []
    per = WARMUP + reps
    for i, (name, A, _, _) in enumerate(shapes()):
        m, K = A.shape
        t = float(np.median(calls[i * per + WARMUP:(i + 1) * per]))
        nbytes = m * (8 * K + 17)
        print(json.dumps({"shape": name, "kernel_ms": t * 1e3, "bytes": nbytes, "hbm_share_at_kernel": nbytes / t / HBM}))


WARMUP = 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--evals-only", action="store_true")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--method", default="iid")
    ap.add_argument("--kernel-trace", help="rocprofv3 kernel_trace.csv of an --evals-only run: report kernel times")
    args = ap.parse_args()
    if args.kernel_trace:
        kernel_shares(args.kernel_trace, args.reps)
        return
    for name, A, b, w in shapes():
        m, K = A.shape
        ctx = _capi.HipContext(0)
        ctx.upload_rows(A, b)
        ctx.set_weights(w)
        r = np.random.default_rng(2)
        c, q = r.standard_normal(K), 0.01 * r.random(K)
        for _ in range(WARMUP):
            ctx.merr_eval(args.method, c, q, 0.1)
        t0 = time.perf_counter()
        for _ in range(args.reps):
            ctx.merr_eval(args.method, c, q, 0.1)
        t_eval = (time.perf_counter() - t0) / args.reps
        nbytes = m * (8 * K + 17)
        rec = {"shape": name, "eval_wall_ms": t_eval * 1e3, "bytes": nbytes,
               "hbm_share_at_wall": nbytes / t_eval / HBM}
        ctx.close()
        if not args.evals_only:
            pt = ParallelTools()
            cfg = Config(pt, {"SOLVER": {"solver": "MERR", "merr_method": args.method, "merr_mult": 0, "merr_cfs": "all"}})
            s = solver_factory.solver("MERR", pt, cfg)
            s.save_files = False
            for timed in (False, True):               # warm-up fit, then the timed one
                np.random.seed(0)
                t0 = time.perf_counter()
                s.perform_fit(A, b, w, trainall=True)
                pt.hip().sync()
                t_fit = time.perf_counter() - t0
            rec.update(fit_wall_s=t_fit, fit_evaluations=s.evaluations, fit_logpost=s.logpost,
                       fit_ms_per_evaluation=t_fit / s.evaluations * 1e3)
            pt.free()
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
