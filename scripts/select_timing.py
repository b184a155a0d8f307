"""Timing of greedy batch selection (fsnap_select_*, kernels of csrc/fsnap_select.hip; Solver.select_batch).

    python scripts/select_timing.py --out profiles/select_timing.txt          # (b), (c): call times per pick
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o sel -- python scripts/select_timing.py --kernels-only
    python scripts/select_timing.py --kernel-trace <dir>/.../sel_kernel_trace.csv --out profiles/select_timing.txt --append

Shapes: 10^6 x 128 with J = 16 and J = 128, 10^6 x 31 (J = 31), 13 035 x 142 (J = 142).
(a) --kernels-only launches, per shape, REPS x [fsnap_select_downdate(V), fsnap_row_variance(NORM, V)] twice over (two
    blocks), so that the kernel trace holds B1 (fsnap_sel_rows_k) next to U1 in NORM form (fsnap_uq_rows_k) at the same
    (K, J) in one run; --kernel-trace reports the median of each per block and the spread between the blocks.
(b) time per pick of Solver.select_batch (8 picks; hipEvents around the synchronous call; the per-pick time is the
    difference to a call with 0 picks, which holds the upload check, begin and the state download), alternating with
(c) the same pick composed from the entry points that existed before the session: fsnap_row_variance(NORM, V) into host
    memory, numpy subtract, bincount, argmax -- with the same host algebra for V and the same sorted row index, built
    once per call.
Pools: configurations of d rows with d = J (J < K) or K ... 300 rows; rows are standard normal, the prior is
tau (A_t^T A_t + I)^-1 of 20 000 training rows."""
import argparse
import csv
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from fitsnap_amd import _capi  # noqa: E402
from fitsnap_amd.config import Config  # noqa: E402
from fitsnap_amd.parallel_tools import ParallelTools  # noqa: E402
from fitsnap_amd.solvers import select, solver_factory  # noqa: E402

SHAPES = [("1e6x128_J16", 1_000_000, 128, 16), ("1e6x128_J128", 1_000_000, 128, 128), ("1e6x31_J31", 1_000_000, 31, 31),
          ("13035x142_J142", 13_035, 142, 142)]
TAU = 0.04
PICKS = 8


def pool(m, K, J, seed=0):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((m, K))
    At = rng.standard_normal((20_000, K))
    C0 = TAU * np.linalg.inv(At.T @ At + np.eye(K))
    sizes = []
    while sum(sizes) < m:
        sizes.append(J if J < K else int(rng.integers(K, 301)))
    sizes[-1] -= sum(sizes) - m
    cat = np.repeat(np.arange(len(sizes)), sizes).astype(np.int32)
    return A, 0.5 * (C0 + C0.T), cat, len(sizes)


def event_ms(fn):
    import torch

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def composed(ctx, A, C0, cat, ncat, picks):
    """PICKS picks from the entry points without a session; returns the picks."""
    out = ctx.row_variance(C0, _capi.UQ_QUAD, cat=cat, ncat=ncat)
    var, sums = out["var"], out["cat_sum"]
    alive = out["cat_count"] > 0
    order = np.argsort(cat, kind="stable")               # the rows of a category, looked up as select_batch does: built once,
    first = np.searchsorted(cat[order], np.arange(ncat + 1))     # so it is part of the time with 0 picks
    C, chosen = C0, []
    for _ in range(picks):
        u = int(np.argmax(np.where(alive, sums, -np.inf)))
        alive[u] = False
        rows = order[first[u]:first[u + 1]]
        V = select.downdate_factor(C, A[rows], TAU)
        C = select.downdate_cov(C, V)
        var -= ctx.row_variance(V, _capi.UQ_NORM)["var"]
        sums = np.bincount(cat, weights=var, minlength=ncat)
        chosen.append(u)
    return chosen


def calls(reps, lines):
    pt = ParallelTools()
    s = solver_factory.solver("ANL", pt, Config(pt, {"SOLVER": {"solver": "ANL"}}))
    lines.append(f"(b) Solver.select_batch / (c) composed from fsnap_row_variance + numpy, {PICKS} picks, alternating, median of {reps}")
    for name, m, K, J in SHAPES:
        A, C0, cat, ncat = pool(m, K, J)
        s.cov = C0
        s.select_batch(1, a=A, categories=cat, noise=TAU)                 # upload + warm-up
        ctx = s._uq_ctx
        composed(ctx, A, C0, cat, ncat, 1)
        tb, t0, tc, tc0 = [], [], [], []
        same = True
        for _ in range(reps):
            t, res = event_ms(lambda: s.select_batch(PICKS, a=A, categories=cat, noise=TAU))
            tb.append(t)
            t0.append(event_ms(lambda: s.select_batch(0, a=A, categories=cat, noise=TAU))[0])
            t, chosen = event_ms(lambda: composed(ctx, A, C0, cat, ncat, PICKS))
            tc.append(t)
            tc0.append(event_ms(lambda: composed(ctx, A, C0, cat, ncat, 0))[0])
            same = same and chosen == res.keys
        b, b0, c, c0 = (float(np.median(x)) for x in (tb, t0, tc, tc0))
        lines.append(f"  {name:16s} ncat {ncat:6d}  (b) {b:9.2f} ms total, {b0:8.2f} ms with 0 picks -> {(b - b0) / PICKS:8.3f} ms / pick   "
                     f"(c) {c:9.2f} ms total, {c0:8.2f} ms with 0 picks -> {(c - c0) / PICKS:8.3f} ms / pick   (c) / (b) per pick "
                     f"{(c - c0) / max(b - b0, 1e-9):6.2f}" + ("" if same else "   (the two batches differ)"))
        print(lines[-1], flush=True)
        del A
    pt.free()


def kernels_only(reps):
    for name, m, K, J in SHAPES:
        A, C0, cat, ncat = pool(m, K, J)
        V = np.random.default_rng(1).standard_normal((K, J)) * 1e-3
        ctx = _capi.HipContext(0)
        ctx.upload_rows(A, np.zeros(m))
        ctx.select_begin(C0, _capi.UQ_QUAD, cat=cat, ncat=ncat)
        for _ in range(2 * reps):
            ctx.select_downdate(V)
            ctx.row_variance(V, _capi.UQ_NORM, want_var=True)
        ctx.close()
        del A


def kernel_times(path, reps, lines):
    """Launch order per shape: 1 fsnap_uq_rows (QUAD, begin), then 2 reps x [fsnap_sel_rows, fsnap_uq_rows (NORM)]."""
    sel, uqr, other = [], [], {}
    with open(path) as f:
        for r in csv.DictReader(f):
            name = r.get("Kernel_Name", "")
            t = (int(r["Start_Timestamp"]), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3)
            if "fsnap_sel_rows" in name:
                sel.append(t)
            elif "fsnap_uq_rows" in name:
                uqr.append(t)
            elif "fsnap_sel_" in name:
                other.setdefault(re.search(r"fsnap_sel_\w+", name).group(0), []).append(t[1])
    sel.sort()
    uqr.sort()
    lines.append(f"(a) kernel times from one rocprofv3 --kernel-trace run, us: median of {reps} launches per block, two blocks per shape")
    for i, (name, m, K, J) in enumerate(SHAPES):
        b1 = [t for _, t in sel[2 * reps * i:2 * reps * (i + 1)]]
        u1 = [t for _, t in uqr[(2 * reps + 1) * i + 1:(2 * reps + 1) * (i + 1)]]
        if len(b1) < 2 * reps or len(u1) < 2 * reps:
            lines.append(f"  {name}: incomplete trace ({len(b1)} / {len(u1)} launches)")
            continue
        mb = [float(np.median(b1[:reps])), float(np.median(b1[reps:]))]
        mu = [float(np.median(u1[:reps])), float(np.median(u1[reps:]))]
        lines.append(f"  {name:16s} B1 fsnap_sel_rows_k {mb[0]:9.1f} / {mb[1]:9.1f}   U1 NORM fsnap_uq_rows_k {mu[0]:9.1f} / {mu[1]:9.1f}   "
                     f"B1 / U1 {np.mean(mb) / np.mean(mu):6.3f}   spread between blocks: B1 {abs(mb[0] - mb[1]) / np.mean(mb) * 100:4.1f} %, "
                     f"U1 {abs(mu[0] - mu[1]) / np.mean(mu) * 100:4.1f} %   min .. max of all launches: B1 {min(b1):.1f} .. {max(b1):.1f}, "
                     f"U1 {min(u1):.1f} .. {max(u1):.1f}")
    for k, v in sorted(other.items()):
        lines.append(f"  {k}: {len(v)} launches, median {float(np.median(v)):.1f} us, max {max(v):.1f} us")
    for line in lines:
        print(line)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--kernel-trace")
    ap.add_argument("--out")
    ap.add_argument("--append", action="store_true")
    a = ap.parse_args()
    out_lines = []
    if a.kernels_only:
        kernels_only(a.reps)
    elif a.kernel_trace:
        kernel_times(a.kernel_trace, a.reps, out_lines)
    else:
        calls(a.reps, out_lines)
    if a.out and out_lines:
        with open(a.out, "a" if a.append else "w") as f:
            f.write("\n".join(out_lines) + "\n")
