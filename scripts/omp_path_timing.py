"""Times of fsnap_omp_path (grouped K-fold greedy sparse-selection paths, csrc/fsnap_omp.hip) next to the host route on the same
downloaded statistics (omp_path.omp_path_host: a pool of 16 Python threads that call fsnap_omp_gram) and next to ONE
scikit-learn orthogonal_mp_gram call on the full system, in the same process, with S = min(64, K) steps and the default ladder
of levels, on two sets of rows:
  - synth: 10^6 x 128 in 6 065 configurations of 30-300 rows;
  - ta:    the golden Ta rows, 15 213 x 31, blocks of 7 consecutive rows as configurations;
each with the configurations dealt into F = 5 folds (folds5), F = 40 (folds40) and every configuration its own fold (loco;
statistics only, no row pass).  Also timed on their own: the layout (fsnap_cat_prepare), the statistics pass (kernel C1,
fsnap_cat_normal_eq), the download of the blocks the host route needs, and the row pass of the per-class table
(fsnap_candidate_rows with F x Q vectors).  Wall-clock times of the synchronous calls (warm: after one call), median of --reps;
the host route of ``loco`` is timed once.  Every case is a child process under its own time limit; after one that did not end
well nothing more is started.

    python scripts/omp_path_timing.py [--reps N] [--out FILE]
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
from fitsnap_amd.solvers import omp_path as op  # noqa: E402

FOLDS = {"folds5": (5, True), "folds40": (40, True), "loco": (None, False)}
CASES = [f"{rows}-{folds}" for rows in ("synth", "ta") for folds in FOLDS]
NCLASS, STEPS, CRITERION = 3, 64, "ols"


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


def case(name, reps, lines):
    which, fname = name.split("-")
    F, row_pass = FOLDS[fname]
    A, b, w, sizes = synth_rows() if which == "synth" else ta_rows()
    m, K = A.shape
    S = min(STEPS, K)
    levels = op.default_levels(S)
    Q = levels.size
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

    def device():
        state["dev"] = ctx.omp_path(state["dptr"], K, F, nsub, CRITERION, (), S, levels)

    def host():
        state["host"] = op.omp_path_host(state["blocks"], K, CRITERION, (), S, levels, nsub)

    t_dev = timed(device, reps)
    t_dev1 = timed(lambda: ctx.omp_path(state["dptr"], K, F, nsub, CRITERION, (), 1, [1]), reps)
    once = fname == "loco"
    t_host = timed(host, 1 if once else reps, warm=0 if once else 1)
    order, path, held, coef = state["dev"]
    same = all(np.array_equal(x, y) for x, y in zip((order, path, coef), (state["host"][0], state["host"][1], state["host"][3])))
    hdiff = float(np.max(np.abs(held[:, :, 1] - state["host"][2][:, :, 1])) / np.max(held[:, :, 2]))
    folds, total = lp.sum_blocks(state["blocks"], nsub)
    Qm, qv, y2, _, _ = lp.downdated(folds, total, F, K)

    def sklearn_call():
        from sklearn.linear_model import orthogonal_mp_gram

        d = np.sqrt(np.diag(Qm))
        orthogonal_mp_gram(Qm / d[:, None] / d[None, :], qv / d, n_nonzero_coefs=S, norms_squared=np.array([y2]), return_path=True)

    t_sk = timed(sklearn_call, reps)
    t_gram = timed(lambda: _capi.omp_gram(Qm, qv, y2, S, CRITERION), reps)
    cv_error, cv_se, best, sparsest = op.cv_picks(np.arange(1, S + 1), held)
    lines.append(f"{name}: m = {m}, K = {K}, {len(sizes)} configurations, F = {F} folds, nsub = {nsub}: {F + 1} problems of S = {S} "
                 f"steps ({CRITERION}), coefficients at Q = {Q} levels; LDS per problem {op_lds(K, S)} B")
    lines.append(f"  layout (fsnap_cat_prepare) {t_prep:.2f} ms   statistics pass C1 (fsnap_cat_normal_eq + one block back) {t_stats:.2f} ms   "
                 f"download of the {ncat} blocks {t_down:.2f} ms")
    lines.append(f"  device route (fsnap_omp_path) {t_dev:.2f} ms (S = 1: {t_dev1:.2f} ms)   host route (omp_path_host: fsnap_omp_gram from "
                 f"{min(lp.HOST_THREADS, os.cpu_count() or 1)} Python threads, without the download) {t_host:.2f} ms   device / host "
                 f"{t_dev / t_host:.3f}")
    lines.append(f"  one problem on the host: fsnap_omp_gram {t_gram:.3f} ms   scikit-learn orthogonal_mp_gram (return_path) {t_sk:.3f} ms")
    lines.append(f"  orders, path rows and level coefficients device == host bit for bit: {same}; largest held-out difference "
                 f"{hdiff:.1e} of the largest bb_f; best {None if best is None else best + 1} terms, fewest within one standard error "
                 f"{None if sparsest is None else sparsest + 1}")
    if row_pass:
        betas = np.ascontiguousarray(coef[:F].reshape(F * Q, K))
        t_rows = timed(lambda: ctx.candidate_rows(state["layout"], betas, None, _capi.CAND_ERROR_SUMS, ncat), reps)
        lines.append(f"  row pass of the per-class table (fsnap_candidate_rows, {F * Q} vectors) {t_rows:.2f} ms")
    ctx.close()


def op_lds(K, S):
    """omp_lds_bytes of csrc/fsnap_omp.hip."""
    return ((S * (K | 1) + 2 * S + K) * 8 + S * 4 + 15) // 16 * 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--case-only", default=None, choices=CASES)
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
