"""Times of fsnap_bcs_path (grouped K-fold BCS sparsity paths, csrc/fsnap_bcs.hip) next to the host route on the same downloaded
statistics (bcs_path.bcs_path_host: a pool of 16 Python threads that call fsnap_bcs_gram) in the same process, with Q = 8
settings (scale 1e-1 ... 1e-6 and two fixed sigma2) of itermax = 80, max_active = min(K, 64), on three sets of rows:
  - synth: 10^6 x 128 in 6 065 configurations of 30-300 rows;
  - ta:    the golden Ta rows, 15 213 x 31, blocks of 7 consecutive rows as configurations;
  - wide:  13 035 x 142 synthetic rows in 1 863 configurations of 7 rows;
each with the configurations dealt into F = 5 folds (folds5) and F = 40 (folds40).  Also timed on their own: the layout
(fsnap_cat_prepare), the statistics pass (kernel C1, fsnap_cat_normal_eq), the download of the blocks the host route needs, the
row pass of the per-class table (fsnap_candidate_rows with F x Q vectors), and the ROW PASSES of one reference-style solve: the
reference's bcs() forms A^T (A_s v) from the rows in every iteration; the script replays, for the fit on all rows of the first
setting, those products in numpy along the picks fsnap_bcs_gram took (no reference code runs here) and SCALES that one problem
to the (F + 1) x Q problems of the call -- labelled "scaled".  Wall-clock times of the synchronous calls (warm: after one call),
median of --reps.  --accuracy adds the largest relative difference between the two routes over the cases of
tests/bcs_cases.py (the figure behind bcs_cases.DEVICE_BAR).  Every case is a child process under its own time limit; after
one that did not end well nothing more is started.

    python scripts/bcs_path_timing.py [--reps N] [--accuracy] [--out FILE]
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
from fitsnap_amd.solvers import bcs_path as bp  # noqa: E402
from fitsnap_amd.solvers import folds as ff  # noqa: E402

FOLDS = {"folds5": 5, "folds40": 40}
CASES = [f"{rows}-{folds}" for rows in ("synth", "ta", "wide") for folds in FOLDS]
NCLASS, ITERMAX = 3, 80
GRID = [{"scale": s, "itermax": ITERMAX} for s in (1e-1, 1e-2, 1e-3, 1e-4, 1e-5, 1e-6)] + \
       [{"sigma2": s, "itermax": ITERMAX} for s in (1e-2, 1e-3)]
SECTION = type("S", (), dict(sigma2=None, scale=0.01, eta=1e-18, itermax=10))


def timed(fn, reps, warm=1):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts))


def synth_rows():
    rng = np.random.default_rng(0)
    sizes = rng.integers(30, 301, 7000)
    sizes = sizes[:int(np.searchsorted(np.cumsum(sizes), 1_000_000)) + 1]
    m, K = int(sizes.sum()), 128
    A = rng.standard_normal((m, K), dtype=np.float64)
    truth = np.where(rng.random(K) < 0.3, rng.standard_normal(K), 0.0)
    b = A @ truth + 0.5 * rng.standard_normal(m)
    w = rng.uniform(0.5, 2.0, m)
    return A, b, w, sizes


def ta_rows():
    z = np.load(os.path.join(ROOT, "tests", "golden", "ta_abw.npz"))
    A, b, w = (np.ascontiguousarray(z[k]) for k in ("A", "b", "w"))
    m = A.shape[0]
    sizes = np.full((m + 6) // 7, 7)
    sizes[-1] = m - 7 * (len(sizes) - 1)
    return A, b, w, sizes


def wide_rows():
    rng = np.random.default_rng(2)
    m, K = 13035, 142
    sizes = np.full((m + 6) // 7, 7)
    sizes[-1] = m - 7 * (len(sizes) - 1)
    A = rng.standard_normal((m, K))
    truth = np.where(rng.random(K) < 0.3, rng.standard_normal(K), 0.0)
    b = A @ truth + 0.5 * rng.standard_normal(m)
    w = rng.uniform(0.5, 2.0, m)
    return A, b, w, sizes


def row_passes(aw, bw, fit):
    """The products with the rows that a row-form BCS solve makes along ``fit``'s picks: A^T y and the column norms at the
    start, then per iteration A^T (A_s v) (re-estimate, delete) or A_s^T a_i and A^T (a_i - A_s v) (add)."""
    aw.T @ bw
    np.einsum("ij,ij->j", aw, aw)
    support = [int(j) for j in fit.active[:1]]             # the initial column (a cost model: deletions may have moved it)
    for j, action in fit.picks:
        if j < 0:
            break
        As = aw[:, support]
        v = np.ones(len(support))
        if action == _capi.BCS_ADD:
            ai = aw[:, j]
            As.T @ ai
            aw.T @ (ai - As @ v)
            support.append(int(j))
        elif action in (_capi.BCS_RE, _capi.BCS_DEL):
            aw.T @ (As @ v)
            if action == _capi.BCS_DEL and int(j) in support:
                support.remove(int(j))
    if support:
        bw - aw[:, support] @ np.ones(len(support))


def differences(dev, host):
    """(fit, heldout): the largest relative differences between the routes' values, each relative to the largest entry of the
    problem's output.  fit: coefficients, alpha, errbars, the scalars sigma2 used / sigma2 re-estimated / rss, and Sig; heldout:
    the held-out error bb_f - 2 beta . c_f + beta^T G_f beta, whose terms cancel to bb_f / h of their size and which the two
    routes add up in different orders.  tests/test_gpu_bcs_path.py holds both within bcs_cases.DEVICE_BAR."""
    worst = [0.0, 0.0]

    def take(x, y, k):
        x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
        scale = np.max(np.abs(y)) if y.size else 0.0
        if scale > 0:
            worst[k] = max(worst[k], float(np.max(np.abs(x - y)) / scale))

    nprob, Q = dev[0].shape[0], dev[0].shape[1]
    for f in range(nprob):
        for q in range(Q):
            for i in (0, 2, 3):                              # coef, alpha, errbars
                take(dev[i][f, q], host[i][f, q], 0)
            for j in (2, 3, 4):                              # sigma2 used, sigma2 re-estimated, rss
                take(dev[5][f, q, j], host[5][f, q, j], 0)
            if f < nprob - 1:
                take(dev[6][f, q, 1], host[6][f, q, 1], 1)
            else:
                take(dev[7][q], host[7][q], 0)
    return worst[0], worst[1]


def largest_difference(dev, host):
    """The larger of ``differences``."""
    return max(differences(dev, host))


def case(name, reps, lines):
    which, fname = name.split("-")
    F = FOLDS[fname]
    A, b, w, sizes = {"synth": synth_rows, "ta": ta_rows, "wide": wide_rows}[which]()
    m, K = A.shape
    grid = bp.resolve_grid(GRID, SECTION)
    hyper = bp.hyper_of(grid)
    Q, MA = len(grid), min(K, bp.MAX_ACTIVE)
    cfg = np.repeat(np.arange(len(sizes)), sizes)
    fold = np.random.default_rng(1).permutation(len(sizes))[cfg] % F
    nsub = NCLASS
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
        state["blocks"] = ff.download_blocks(ctx, state["dptr"], ncat, K)

    t_prep = timed(prepare, reps)
    t_stats = timed(stats, reps)
    t_down = timed(download, 1, warm=0)

    def device():
        state["dev"] = ctx.bcs_path(state["dptr"], K, F, nsub, hyper, MA, "reference")

    def host():
        state["host"] = bp.bcs_path_host(state["blocks"], K, hyper, MA, "reference", nsub)

    t_dev = timed(device, reps)
    t_dev1 = timed(lambda: ctx.bcs_path(state["dptr"], K, F, nsub, hyper[:1], MA, "reference"), reps)
    t_host = timed(host, reps)
    dev, hst = state["dev"], state["host"]
    same = np.array_equal(dev[4], hst[4]) and np.array_equal(dev[1], hst[1])
    diff, hdiff = differences(dev, hst)
    cancel = float(np.max(hst[6][:, :, 2] / np.maximum(np.abs(hst[6][:, :, 1]), 1e-300)))
    folds, total = ff.sum_blocks(state["blocks"], nsub)
    Qm, qv, y2, n, _ = ff.downdated(folds, total, F, K)
    sum_y = total[K * K + K + 1]
    g0 = grid[0]
    one = lambda: _capi.bcs_gram(Qm, qv, y2, sum_y, n, g0["sigma2"], g0["scale"], g0["eta"], ITERMAX, MA)   # noqa: E731
    t_gram = timed(one, reps)
    fit = one()
    aw, bw = A * w[:, None], b * w
    t_rows1 = timed(lambda: row_passes(aw, bw, fit), max(1, reps // 2), warm=0)
    nprob = (F + 1) * Q
    info = dev[5]
    na = (dev[1] >= 0).sum(axis=2)
    lines.append(f"{name}: m = {m}, K = {K}, {len(sizes)} configurations, F = {F} folds, nsub = {nsub}: {nprob} problems, Q = {Q} "
                 f"settings of itermax = {ITERMAX}, max_active = {MA}; iterations {int(info[:, :, 0].min())} ... "
                 f"{int(info[:, :, 0].max())}, active columns {int(na.min())} ... {int(na.max())}; LDS per problem "
                 f"{lds_bytes(K, MA)} B")
    lines.append(f"  layout (fsnap_cat_prepare) {t_prep:.2f} ms   statistics pass C1 (fsnap_cat_normal_eq + one block back) {t_stats:.2f} ms   "
                 f"download of the {ncat} blocks {t_down:.2f} ms")
    lines.append(f"  device route (fsnap_bcs_path) {t_dev:.2f} ms (Q = 1: {t_dev1:.2f} ms)   host route (bcs_path_host: fsnap_bcs_gram from "
                 f"{min(ff.HOST_THREADS, os.cpu_count() or 1)} Python threads, without the download) {t_host:.2f} ms   device / host "
                 f"{t_dev / t_host:.3f}")
    lines.append(f"  one problem on the host: fsnap_bcs_gram {t_gram:.3f} ms ({fit.iterations} iterations)   the row passes of one "
                 f"reference-style solve of it, replayed in numpy {t_rows1:.1f} ms; SCALED to {nprob} problems: {t_rows1 * nprob:.0f} ms")
    lines.append(f"  picks and active sets device == host: {same}; smallest margin on the host route {hst[5][:, :, 5].min():.2e}; "
                 f"largest relative difference of the fits (coefficients, alpha, errbars, sigma2, rss, Sig) {diff:.2e}, of the held-out errors "
                 f"{hdiff:.2e} (largest bb_f / h there {cancel:.1e})")
    betas = np.ascontiguousarray(np.nan_to_num(dev[0][:F]).reshape(F * Q, K))
    t_rows = timed(lambda: ctx.candidate_rows(state["layout"], betas, None, _capi.CAND_ERROR_SUMS, ncat), reps)
    lines.append(f"  row pass of the per-class table (fsnap_candidate_rows, {F * Q} vectors) {t_rows:.2f} ms")
    ctx.close()


def lds_bytes(K, MA):
    """bcs_lds_bytes of csrc/fsnap_bcs.hip."""
    return (MA * (MA | 1) + MA * (K | 1) + 4 * MA + K + 8 + 4) * 8 + (MA + 4 + 2) * 4


def accuracy(lines):
    """Device against host route over the path cases of tests/bcs_cases.py (one context, the blocks uploaded by torch)."""
    import torch

    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import bcs_cases as cs

    ctx = _capi.HipContext(0)
    worst = (0.0, None)
    for name in cs.PATH_CASES:
        blocks, K, F, nsub, hyper, ma, deletion = cs.case_blocks(name)
        t = torch.from_numpy(np.array(blocks, dtype=np.float64, order="C")).to("cuda:0")
        torch.cuda.synchronize()
        dev = ctx.bcs_path(t.data_ptr(), K, F, nsub, hyper, ma, deletion)
        host = cs.case_host(name)
        d = largest_difference(dev, host)
        same = np.array_equal(dev[4], host[4])
        lines.append(f"  {name}: K = {K}, F = {F}, Q = {hyper.shape[0]}, max_active = {ma}, {deletion}: picks equal {same}, largest "
                     f"relative difference {d:.3e}, smallest margin {host[5][:, :, 5].min():.2e}")
        if d > worst[0]:
            worst = (d, name)
        del t
    ctx.close()
    lines.insert(0, f"accuracy: device against host route on the same statistics over the cases of tests/bcs_cases.py: largest "
                    f"relative difference {worst[0]:.3e} ({worst[1]}); bcs_cases.DEVICE_BAR is 100 x the figure measured there")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--case-only", default=None, choices=CASES + ["accuracy"])
    ap.add_argument("--accuracy", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.case_only:
        lines = []
        if args.case_only == "accuracy":
            accuracy(lines)
        else:
            case(args.case_only, args.reps, lines)
        print("\n".join(lines))
        return 0
    lines, rc = [], 0
    for name in (["accuracy"] if args.accuracy else []) + CASES:
        r = subprocess.run(["timeout", "-k", "10", "400", sys.executable, os.path.abspath(__file__), "--case-only", name, "--reps",
                            str(args.reps)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        rc = r.returncode
        if rc != 0:
            lines.append(f"{name}: the timing step ended with status {rc}")
            lines.append((r.stdout + r.stderr)[-2000:])
            break
        lines.append(r.stdout.rstrip())
        print(lines[-1], flush=True)
    text = "\n".join(lines)
    if rc != 0:
        print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
