"""Times of fsnap_loco_rows_uq (leave-one-configuration-out predictive variances, csrc/fsnap_loco_uq.hip) next to
fsnap_loco_rows at the shape of profiles/loco_timing.txt: 10^6 x 128 in 6 065 configurations of 30-300 rows (RIDGE factor of
the synthetic rows).  All in one process and run: the median of --reps warm synchronous calls of either entry, and
loco_uq_host on a 1 % sample of the configurations, scaled to all of them (labelled as scaled).

    python scripts/loco_uq_timing.py [--reps N] [--out FILE]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from fitsnap_amd import _capi  # noqa: E402
from fitsnap_amd.solvers import loco, loco_uq  # noqa: E402


def timed(fn, reps):
    fn()
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    sizes = rng.integers(30, 301, 7000)
    sizes = sizes[:int(np.searchsorted(np.cumsum(sizes), 1_000_000)) + 1]     # the first configurations that reach 10^6 rows
    m, K = int(sizes.sum()), 128
    A = rng.standard_normal((m, K))
    b = A @ rng.standard_normal(K) + 0.05 * rng.standard_normal(m)
    w = rng.uniform(0.5, 2.0, m)
    Aw = A * w[:, None]
    G = Aw.T @ Aw
    beta = np.linalg.solve(G + 1e-8 * np.eye(K), Aw.T @ (b * w))
    M = loco.factor_cholesky(G, 1e-8)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    rows = np.arange(m, dtype=np.int32)
    ctx = _capi.HipContext(0)
    ctx.upload_rows(A, b)
    ctx.set_weights(w)
    t_uq = timed(lambda: ctx.loco_rows_uq(M, beta, rows, off), args.reps)
    t_loco = timed(lambda: ctx.loco_rows(M, beta, rows, off), args.reps)
    pred, lev, info = ctx.loco_rows_uq(M, beta, rows, off)
    pred0, _ = ctx.loco_rows(M, beta, rows, off)
    ctx.close()
    pick = np.sort(rng.choice(len(sizes), max(len(sizes) // 100, 1), replace=False))
    srows = np.concatenate([rows[off[u]:off[u + 1]] for u in pick]).astype(np.int32)
    soff = np.concatenate([[0], np.cumsum(sizes[pick])]).astype(np.int64)
    t0 = time.perf_counter()
    hpred, hlev, hinfo = loco_uq.loco_uq_host(A, b, w, M, beta, srows, soff)
    t_host = 1e3 * (time.perf_counter() - t0)
    d = info[:, 0]
    bins = [int((d <= 32).sum()), int(((d > 32) & (d <= 64)).sum()), int(((d > 64) & (d <= 128)).sum()), int((d > 128).sum())]
    lines = [
        f"m = {m}, K = J = {K}, {len(sizes)} configurations of {int(sizes.min())}-{int(sizes.max())} rows; d_c bins <=32 / <=64 / "
        f"<=128 / general: {bins}; n space {int(info[:, 3].sum())}; median of {args.reps} warm calls",
        f"  fsnap_loco_rows_uq call {t_uq:.3f} ms   fsnap_loco_rows call {t_loco:.3f} ms   ratio {t_uq / t_loco:.2f} (goal: at most 3)",
        f"  loco_uq_host on {len(pick)} configurations ({int(soff[-1])} rows) {t_host:.1f} ms: SCALED to all rows "
        f"{t_host * m / soff[-1]:.0f} ms, {t_host * m / soff[-1] / t_uq:.0f} x the device call",
        f"  predictions equal fsnap_loco_rows's bit for bit: {np.array_equal(pred, pred0)}; device against host on the sample: "
        f"max |q - q_host| / q_host {np.max(np.abs(lev[srows] - hlev[srows]) / hlev[srows]):.2e}, "
        f"max |D - D_host| / D_host {np.max(np.abs(info[pick, 5] - hinfo[:, 5]) / hinfo[:, 5]):.2e}, "
        f"max |l - l_host| {np.max(np.abs(info[pick, 4] - hinfo[:, 4])):.2e}",
    ]
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
