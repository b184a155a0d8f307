"""Times of fsnap_loco_rows (leave-one-configuration-out predictions, csrc/fsnap_loco.hip) next to one fsnap_row_variance
NORM call at the same shape:
  - 10^6 x 128, configurations of 30-300 rows (RIDGE factor of the synthetic rows);
  - 15 213 x 31, the golden Ta rows, configurations of 7 rows and the five groups.
Call times are wall-clock times of the synchronous library call (warm: after two calls), median of --reps.  Kernel times
come from a run of its own under rocprofv3 --kernel-trace --stats (fsnap_loco_zeta_k, fsnap_loco_cfg_k<D>).

    python scripts/loco_timing.py [--reps N] [--out FILE]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from fitsnap_amd import _capi  # noqa: E402
from fitsnap_amd.solvers import loco  # noqa: E402


def timed(fn, reps):
    fn()
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts))


def case(name, A, b, w, sizes, reps, lines):
    K = A.shape[1]
    Aw = A * w[:, None]
    G = Aw.T @ Aw
    beta = np.linalg.solve(G + 1e-8 * np.eye(K), Aw.T @ (b * w))
    M = loco.factor_cholesky(G, 1e-8)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    rows = np.arange(len(b), dtype=np.int32)
    ctx = _capi.HipContext(0)
    ctx.upload_rows(A, b)
    ctx.set_weights(w)
    t_loco = timed(lambda: ctx.loco_rows(M, beta, rows, off), reps)
    _, info = ctx.loco_rows(M, beta, rows, off)
    t_norm = timed(lambda: ctx.row_variance(M, _capi.UQ_NORM), reps)
    d = info[:, 0]
    bins = [(d <= 32).sum(), ((d > 32) & (d <= 64)).sum(), ((d > 64) & (d <= 128)).sum(), (d > 128).sum()]
    zeta_flop = 2.0 * len(b) * K * K
    lines.append(f"{name}: m = {len(b)}, K = J = {K}, {len(sizes)} configurations of {int(np.min(sizes))}-{int(np.max(sizes))} "
                 f"rows; d_c bins <=32 / <=64 / <=128 / general: {bins}; n space {int(info[:, 3].sum())}")
    lines.append(f"  fsnap_loco_rows call {t_loco:.3f} ms   fsnap_row_variance NORM call {t_norm:.3f} ms   ratio {t_loco / t_norm:.2f}")
    lines.append(f"  zeta pass alone: {zeta_flop / 1e9:.2f} GFLOP, MFMA bound {zeta_flop / 78.6e12 * 1e3:.3f} ms at 78.6 TF/s")
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []
    rng = np.random.default_rng(0)
    sizes = rng.integers(30, 301, 7000)
    sizes = sizes[:int(np.searchsorted(np.cumsum(sizes), 1_000_000)) + 1]     # the first configurations that reach 10^6 rows
    m = int(sizes.sum())
    A = rng.standard_normal((m, 128))
    b = A @ rng.standard_normal(128) + 0.05 * rng.standard_normal(m)
    w = rng.uniform(0.5, 2.0, m)
    case("synthetic", A, b, w, sizes, args.reps, lines)
    del A, b, w
    z = np.load(os.path.join(ROOT, "tests", "golden", "ta_abw.npz"))
    A, b, w = (np.ascontiguousarray(z[k]) for k in ("A", "b", "w"))
    sizes = np.full(len(b) // 7, 7)
    sizes[-1] += len(b) - sizes.sum()
    case("Ta, 7-row configurations", A, b, w, sizes, args.reps, lines)
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
