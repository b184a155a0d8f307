"""Timing of the predictive-variance pass (fsnap_row_variance, kernels U1 / U1G of csrc/fsnap_uq.hip).

    python scripts/uq_timing.py                      # call times (events around the call) and the numpy expression
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o uq -- python scripts/uq_timing.py --calls-only
    python scripts/uq_timing.py --kernel-trace <dir>/uq_kernel_trace.csv   # kernel times -> share of the bounds

Shapes: 10^6 x 128 (QUAD, NORM J = 128, sam J = 133), 10^6 x 31, 15 213 x 31, 13 035 x 142, 15 213 x 1 595 (QUAD unless
named).  Bounds: the MFMA bound 2 m K J / 78.6 TF (fp64 matrix peak) and the HBM bound 8 m K / 8 TB/s; the larger one
binds.  Call time: hipEvents (torch.cuda.Event) around the synchronous host call, var downloaded, median of --reps.
numpy: the expression (A @ C * A).sum(-1) (QUAD) or ((A @ M) ** 2).sum(-1) (NORM) on the host BLAS with
OMP_NUM_THREADS threads, median of 3."""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from fitsnap_amd import _capi  # noqa: E402

MFMA = 78.6e12
HBM = 8.0e12
SHAPES = [("1e6x128_quad", 1_000_000, 128, 128, 0), ("1e6x128_norm", 1_000_000, 128, 128, 1),
          ("1e6x128_sam133", 1_000_000, 128, 133, 1), ("1e6x31_quad", 1_000_000, 31, 31, 0),
          ("15213x31_quad", 15_213, 31, 31, 0), ("13035x142_quad", 13_035, 142, 142, 0),
          ("15213x1595_quad", 15_213, 1595, 1595, 0)]


def bounds(m, K, J):
    return 2.0 * m * K * J / MFMA * 1e3, 8.0 * m * K / HBM * 1e3


def run(reps, calls_only):
    import torch

    rng = np.random.default_rng(0)
    out = []
    for name, m, K, J, mode in SHAPES:
        A = rng.standard_normal((m, K))
        X = rng.standard_normal((K + 3, K))
        M = X.T @ X / (K + 3) if mode == 0 else rng.standard_normal((K, J))
        ctx = _capi.HipContext(0)
        ctx.upload_rows(A, np.zeros(m))
        ctx.row_variance(M, mode)                   # warm-up
        ts = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ctx.row_variance(M, mode)
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        rec = {"shape": name, "m": m, "K": K, "J": J, "mode": "QUAD" if mode == 0 else "NORM", "call_ms": float(np.median(ts))}
        if not calls_only:
            tn = []
            for _ in range(3):
                t0 = time.perf_counter()
                T = A @ M
                _ = (T * A).sum(-1) if mode == 0 else (T * T).sum(-1)
                tn.append((time.perf_counter() - t0) * 1e3)
            rec["numpy_ms"] = float(np.median(tn))
            rec["numpy_threads"] = os.environ.get("OMP_NUM_THREADS", "default")
            rec["speedup_call"] = rec["numpy_ms"] / rec["call_ms"]
        bm, bh = bounds(m, K, J)
        rec.update(mfma_bound_ms=bm, hbm_bound_ms=bh, binds="MFMA" if bm >= bh else "HBM")
        print(json.dumps(rec), flush=True)
        out.append(rec)
        ctx.close()
        del A
    return out


def kernel_times(path, reps):
    """Per shape (in launch order: 1 warm-up + reps launches of the row kernel per shape), the median kernel time."""
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            if "fsnap_uq_rows" in r.get("Kernel_Name", ""):
                rows.append((int(r["Start_Timestamp"]), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6))
    rows.sort()
    per = reps + 1
    for i, (name, m, K, J, mode) in enumerate(SHAPES):
        ks = [t for _, t in rows[i * per + 1:(i + 1) * per]]
        if not ks:
            break
        k = float(np.median(ks))
        bm, bh = bounds(m, K, J)
        b = max(bm, bh)
        print(json.dumps({"shape": name, "kernel_ms": k, "bound_ms": b, "binds": "MFMA" if bm >= bh else "HBM",
                          "share_of_bound": b / k}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--calls-only", action="store_true")
    ap.add_argument("--kernel-trace")
    a = ap.parse_args()
    if a.kernel_trace:
        kernel_times(a.kernel_trace, a.reps)
    else:
        run(a.reps, a.calls_only)
