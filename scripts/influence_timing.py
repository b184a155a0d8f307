"""Times of fsnap_influence_rows (influence vectors and the sums of the cluster-robust covariances, csrc/fsnap_influence.hip)
at the shape of profiles/loco_timing.txt: 10^6 x 128 in 6 065 configurations of 30-300 rows (RIDGE factor of the synthetic
rows).  All in one process and run, the median of --reps warm synchronous calls of every entry: FULL mode against
fsnap_loco_rows_uq (goal: at most 1.25 x), SCORES mode (with W_s, and without vectors and sums: kernels L1 and I0 alone, the
nearest a host timer gets to fsnap_loco_rows' L1 share) next to fsnap_loco_rows, and influence_host on a 1 % sample of the
configurations, scaled to all of them (labelled as scaled).

    python scripts/influence_timing.py [--reps N] [--out FILE]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from fitsnap_amd import _capi  # noqa: E402
from fitsnap_amd.solvers import influence, loco  # noqa: E402


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
    t_full = timed(lambda: ctx.influence_rows(M, beta, rows, off), args.reps)
    t_full_lean = timed(lambda: ctx.influence_rows(M, beta, rows, off, want_vectors=False), args.reps)
    t_uq = timed(lambda: ctx.loco_rows_uq(M, beta, rows, off), args.reps)
    t_loco = timed(lambda: ctx.loco_rows(M, beta, rows, off), args.reps)
    t_scores = timed(lambda: ctx.influence_rows(M, beta, rows, off, mode=_capi.INFL_SCORES, want_vectors=False), args.reps)
    t_scores_bare = timed(lambda: ctx.influence_rows(M, beta, rows, off, mode=_capi.INFL_SCORES, want_vectors=False,
                                                     want_sums=False), args.reps)
    out = ctx.influence_rows(M, beta, rows, off)
    sc = ctx.influence_rows(M, beta, rows, off, mode=_capi.INFL_SCORES)
    pred0, _ = ctx.loco_rows(M, beta, rows, off)
    ctx.close()
    pick = np.sort(rng.choice(len(sizes), max(len(sizes) // 100, 1), replace=False))
    srows = np.concatenate([rows[off[u]:off[u + 1]] for u in pick]).astype(np.int32)
    soff = np.concatenate([[0], np.cumsum(sizes[pick])]).astype(np.int64)
    t0 = time.perf_counter()
    host = influence.influence_host(A, b, w, M, beta, srows, soff)
    t_host = 1e3 * (time.perf_counter() - t0)
    vs = np.max(np.abs(out["V"][pick] - host["V"])) / np.max(np.abs(host["V"]))
    ss = np.max(np.abs(out["S"][pick] - host["S"])) / np.max(np.abs(host["S"]))
    lines = [
        f"m = {m}, K = J = {K}, {len(sizes)} configurations of {int(sizes.min())}-{int(sizes.max())} rows; n space "
        f"{int(out['info'][:, 3].sum())}; median of {args.reps} warm calls",
        f"  fsnap_influence_rows FULL (pred, V, S, W_s, W_v) {t_full:.3f} ms, without the downloads of V and S {t_full_lean:.3f} ms"
        f"   fsnap_loco_rows_uq {t_uq:.3f} ms   fsnap_loco_rows {t_loco:.3f} ms",
        f"  FULL / fsnap_loco_rows_uq = {t_full / t_uq:.2f} (goal: at most 1.25: {'met' if t_full <= 1.25 * t_uq else 'MISSED'})",
        f"  fsnap_influence_rows SCORES (W_s) {t_scores:.3f} ms, kernels L1 + I0 alone {t_scores_bare:.3f} ms (goal: near the zeta "
        f"pass, 0.91 ms at the last record, plus launch latency and the uploads of M, the index and the offsets)",
        f"  influence_host on {len(pick)} configurations ({int(soff[-1])} rows) {t_host:.1f} ms: SCALED to all rows "
        f"{t_host * m / soff[-1]:.0f} ms, {t_host * m / soff[-1] / t_full:.0f} x the FULL call",
        f"  predictions equal fsnap_loco_rows's bit for bit: {np.array_equal(out['pred'], pred0)}; S and W_s of SCORES equal FULL's "
        f"bit for bit: {np.array_equal(sc['S'], out['S']) and np.array_equal(sc['Ws'], out['Ws'])}; device against host on the "
        f"sample: max |V - V_host| / max |V_host| {vs:.2e}, max |S - S_host| / max |S_host| {ss:.2e}",
    ]
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
