"""Times of fsnap_ridge_path (leave-one-unit-out refits over a grid of alphas, csrc/fsnap_path.hip) next to the composed route
on the same context, Q x (loco.factor_cholesky + fsnap_loco_rows), at the two shapes of profiles/loco_timing.txt:
  - 10^6 x 128 in units of 30-300 rows, Q = 16;
  - 15 213 x 31, the golden Ta rows in units of 7 rows, Q = 16.
Call times are wall-clock times of the synchronous calls (warm: after two calls), median of --reps.  The share of the
alpha-dependent part of the kernel (scaling, factorisation, the two solves) is estimated from the calls with Q = 16 and
Q = 1: 16 (t16 - t1) / (15 t16).  Kernel times come from a run of its own under rocprofv3 --kernel-trace --stats (--profile).
Every step (the wall-clock timing of a shape, the profiled run of a shape) is a child process under its own time limit; the
profiled ones come last, and after a step that did not end well nothing more is started.

    python scripts/ridge_path_timing.py [--reps N] [--profile] [--out FILE]
"""
import argparse
import csv
import glob
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from fitsnap_amd import _capi  # noqa: E402
from fitsnap_amd.solvers import loco  # noqa: E402

ALPHAS = np.logspace(-10, 2, 16)


def timed(fn, reps):
    fn()
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts))


def shape(name):
    rng = np.random.default_rng(0)
    if name == "synthetic":
        sizes = rng.integers(30, 301, 7000)
        sizes = sizes[:int(np.searchsorted(np.cumsum(sizes), 1_000_000)) + 1]
        m = int(sizes.sum())
        A = rng.standard_normal((m, 128))
        b = A @ rng.standard_normal(128) + 0.05 * rng.standard_normal(m)
        w = rng.uniform(0.5, 2.0, m)
        return A, b, w, sizes
    z = np.load(os.path.join(ROOT, "tests", "golden", "ta_abw.npz"))
    A, b, w = (np.ascontiguousarray(z[k]) for k in ("A", "b", "w"))
    sizes = np.full(len(b) // 7, 7)
    sizes[-1] += len(b) - sizes.sum()
    return A, b, w, sizes


def setup(name):
    A, b, w, sizes = shape(name)
    Aw = A * w[:, None]
    G, c = Aw.T @ Aw, Aw.T @ (b * w)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    rows = np.arange(len(b), dtype=np.int32)
    cls = (np.arange(len(b)) % 3).astype(np.uint8)
    ctx = _capi.HipContext(0)
    ctx.upload_rows(A, b)
    ctx.set_weights(w)
    return ctx, G, c, rows, off, cls, sizes


def composed(ctx, G, c, rows, off):
    for alpha in ALPHAS:
        M = loco.factor_cholesky(G, alpha)
        ctx.loco_rows(M, M @ (M.T @ c), rows, off)


def case(name, reps, lines):
    ctx, G, c, rows, off, cls, sizes = setup(name)
    K = G.shape[0]
    t16 = timed(lambda: ctx.ridge_path(G, c, ALPHAS, rows, off, cls, 3), reps)
    t1 = timed(lambda: ctx.ridge_path(G, c, ALPHAS[:1], rows, off, cls, 3), reps)
    tp = timed(lambda: ctx.ridge_path(G, c, ALPHAS, rows, off, cls, 3, want_preds=True), reps)
    tc = timed(lambda: composed(ctx, G, c, rows, off), reps)
    tl = timed(lambda: ctx.loco_rows(loco.factor_cholesky(G, 1e-8), np.zeros(K), rows, off), reps)
    share = 16.0 * (t16 - t1) / (15.0 * t16)
    lines.append(f"{name}: m = {len(rows)}, K = {K}, {len(sizes)} units of {int(np.min(sizes))}-{int(np.max(sizes))} rows, "
                 f"Q = {len(ALPHAS)}")
    lines.append(f"  fsnap_ridge_path call {t16:.3f} ms (Q = 1: {t1:.3f} ms; with the Q x m predictions: {tp:.3f} ms)")
    lines.append(f"  composed route, Q x (factor_cholesky + fsnap_loco_rows): {tc:.3f} ms (one factor + call: {tl:.3f} ms)")
    lines.append(f"  fused / composed: {t16 / tc:.3f}   alpha-dependent share of the fused call (scaling, factorisation, "
                 f"solves): {share:.2f}")
    ctx.close()


def calls_only(name):
    ctx, G, c, rows, off, cls, _ = setup(name)
    for _ in range(3):
        ctx.ridge_path(G, c, ALPHAS, rows, off, cls, 3)
    composed(ctx, G, c, rows, off)
    ctx.close()


def step(args, limit):
    """One step in a child process of its own under its own time limit: (status, output)."""
    cmd = ["timeout", "-k", "10", str(limit), *args]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    return r.returncode, r.stdout if r.returncode == 0 else r.stdout + r.stderr


def profile(name, lines, limit):
    with tempfile.TemporaryDirectory() as d:
        rc, _ = step(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "path", "--",
                      sys.executable, os.path.abspath(__file__), "--calls-only", name], limit)
        if rc != 0:
            lines.append(f"  rocprofv3 run of {name} ended with status {rc}: no kernel times")
            return rc
        lines.append(f"{name}, kernel times (rocprofv3 --kernel-trace --stats, a run of its own):")
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            with open(path, newline="") as f:
                for row in csv.DictReader(f):
                    kname = row.get("Name", "")
                    found = re.search(r"fsnap_(path|loco)\w*(<\d+>)?", kname)
                    if found:
                        calls = int(row.get("Calls", 0) or 0)
                        avg = float(row.get("AverageNs", 0.0) or 0.0)
                        lines.append(f"  kernel {found.group(0)}: {calls} calls, {avg / 1e6:.3f} ms each")
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--calls-only", default=None, choices=["synthetic", "ta"])
    ap.add_argument("--case-only", default=None, choices=["synthetic", "ta"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.calls_only:
        calls_only(args.calls_only)
        return 0
    if args.case_only:
        lines = []
        case(args.case_only, args.reps, lines)
        print("\n".join(lines))
        return 0
    # every step is a process of its own under its own time limit; the wall-clock steps first, the profiled ones last; after
    # a step that did not end well nothing more is started on the GPU: what was collected is written and the script ends
    lines = []
    rc = 0
    for name in ("synthetic", "ta"):
        rc, out = step([sys.executable, os.path.abspath(__file__), "--case-only", name, "--reps", str(args.reps)], 300)
        if rc != 0:
            lines.append(f"{name}: the timing step ended with status {rc}")
            lines.append(out[-2000:])
            break
        lines.append(out.rstrip())
    if rc == 0 and args.profile:
        for name in ("synthetic", "ta"):
            rc = profile(name, lines, 300)
            if rc != 0:
                break
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
