"""Times of fsnap_lasso_path (grouped K-fold LASSO alpha paths, csrc/fsnap_lasso.hip) next to the host route on the same
downloaded statistics (lasso_path.lasso_path_host: a pool of 16 Python threads that call fsnap_lasso_gram; the numpy
downdates and the wrapper's work around every solve hold the interpreter lock), in the same process, on 10^6 x 128 rows
in 6 065 configurations of 30-300 rows:
  - folds5:   the configurations dealt into F = 5 folds, Q = 16;
  - groups40: F = 40 groups, Q = 16;
  - loco:     every configuration its own fold (F = 6 065), Q = 8, statistics only (no row pass).
Also timed on their own: the layout (fsnap_cat_prepare), the statistics pass (kernel C1, fsnap_cat_normal_eq), the download of
the blocks the host route needs, and the row pass of the per-class table (fsnap_candidate_rows with F x Q vectors).  Wall-clock
times of the synchronous calls (warm: after one call), median of --reps; the host route of ``loco`` is timed once.  Every case
is a child process under its own time limit; after one that did not end well nothing more is started.

    python scripts/lasso_path_timing.py [--reps N] [--out FILE]
"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from fitsnap_amd import _capi  # noqa: E402
from fitsnap_amd.solvers import lasso_path as lp  # noqa: E402

CASES = {"folds5": (5, 16, True), "groups40": (40, 16, True), "loco": (None, 8, False)}
TOL, MAX_ITER, NCLASS = 1e-4, 2000, 3


def timed(fn, reps, warm=1):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts))


def rows():
    rng = np.random.default_rng(0)
    sizes = rng.integers(30, 301, 7000)
    sizes = sizes[:int(np.searchsorted(np.cumsum(sizes), 1_000_000)) + 1]
    m, K = int(sizes.sum()), 128
    A = rng.standard_normal((m, K), dtype=np.float64)
    truth = np.where(rng.random(K) < 0.3, rng.standard_normal(K), 0.0)
    b = A @ truth + 0.5 * rng.standard_normal(m)
    w = rng.uniform(0.5, 2.0, m)
    return A, b, w, sizes


def case(name, reps, lines):
    F, Q, row_pass = CASES[name]
    A, b, w, sizes = rows()
    m, K = A.shape
    cfg = np.repeat(np.arange(len(sizes)), sizes)
    if F is None:
        F, fold = len(sizes), cfg
    else:
        fold = np.random.default_rng(1).permutation(len(sizes))[cfg] % F
    nsub = NCLASS if row_pass else 1
    cat = (fold * nsub + (np.arange(m) % nsub)).astype(np.int32)
    ncat, T = F * nsub, K * K + K + 3
    ctx = _capi.HipContext(0)
    ctx.upload_rows(A, b)
    ctx.set_weights(w)
    state = {}

    def prepare():
        state["layout"] = ctx.cat_prepare(cat, ncat)

    def stats():
        state["dptr"] = ctx.cat_normal_eq(state["layout"])
        ctx.download_packed(state["dptr"], K)              # the call only queues the kernels: wait for them (one block back)

    def download():
        blocks = np.empty((ncat, T))
        for i in range(ncat):
            G, c, s = ctx.download_packed(state["dptr"] + i * T * 8, K)
            blocks[i, :K * K], blocks[i, K * K:K * K + K], blocks[i, K * K + K:] = G.ravel(), c, s
        state["blocks"] = blocks

    t_prep = timed(prepare, reps)
    t_stats = timed(stats, reps)
    t_down = timed(download, 1, warm=0)
    _, total = lp.sum_blocks(state["blocks"], nsub)
    _, c, _, n = lp.unpack(total, K)
    alphas = float(np.max(np.abs(c))) / n * np.logspace(-0.5, -4.0, Q)

    def device():
        state["dev"] = ctx.lasso_path(state["dptr"], K, F, nsub, alphas, MAX_ITER, TOL)

    def host():
        state["host"] = lp.lasso_path_host(state["blocks"], K, alphas, MAX_ITER, TOL, nsub)

    t_dev = timed(device, reps)
    t_dev1 = timed(lambda: ctx.lasso_path(state["dptr"], K, F, nsub, alphas[:1], MAX_ITER, TOL), reps)
    t_host = timed(host, 1 if name == "loco" else reps, warm=0 if name == "loco" else 1)
    coef, info, held = state["dev"]
    diff = float(np.max(np.abs(coef - state["host"][0])) / np.max(np.abs(coef)))
    lines.append(f"{name}: m = {m}, K = {K}, {len(sizes)} configurations, F = {F} folds, Q = {Q}, nsub = {nsub}: "
                 f"{(F + 1) * Q} problems, tol = {TOL:g}")
    lines.append(f"  layout (fsnap_cat_prepare) {t_prep:.2f} ms   statistics pass C1 (fsnap_cat_normal_eq + one block back) {t_stats:.2f} ms   "
                 f"download of the {ncat} blocks {t_down:.2f} ms")
    lines.append(f"  device route (fsnap_lasso_path) {t_dev:.2f} ms (Q = 1: {t_dev1:.2f} ms)   host route (lasso_path_host: fsnap_lasso_gram from "
                 f"{min(lp.HOST_THREADS, os.cpu_count() or 1)} Python threads, without the download) {t_host:.2f} ms   device / host "
                 f"{t_dev / t_host:.3f}")
    lines.append(f"  sweeps: median {int(np.median(info[:, :, 0]))}, max {int(info[:, :, 0].max())}; non-zero coefficients of the "
                 f"full fits {np.count_nonzero(coef[F], axis=1).min()}-{np.count_nonzero(coef[F], axis=1).max()}; largest "
                 f"difference device - host {diff:.1e} of the largest coefficient")
    if row_pass:
        betas = np.ascontiguousarray(coef[:F].reshape(F * Q, K))
        t_rows = timed(lambda: ctx.candidate_rows(state["layout"], betas, None, _capi.CAND_ERROR_SUMS, ncat), reps)
        lines.append(f"  row pass of the per-class table (fsnap_candidate_rows, {F * Q} vectors) {t_rows:.2f} ms")
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--case-only", default=None, choices=list(CASES))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.case_only:
        lines = []
        case(args.case_only, args.reps, lines)
        print("\n".join(lines))
        return 0
    lines, rc = [], 0
    for name in CASES:
        r = subprocess.run(["timeout", "-k", "10", "400", sys.executable, os.path.abspath(__file__), "--case-only", name, "--reps",
                            str(args.reps)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        rc = r.returncode
        if rc != 0:
            lines.append(f"{name}: the timing step ended with status {rc}")
            lines.append((r.stdout + r.stderr)[-2000:])
            break
        lines.append(r.stdout.rstrip())
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
