"""Times of fsnap_spectral_path (grouped K-fold spectral paths, csrc/fsnap_spectral.hip) with Q = 256 settings (64 alphas x 4
rconds), kernels E1 (eigendecompositions) and E2 (settings) separately by HIP events, next to, in the same process and over the
same statistics:
  - the host route (spectral_path.spectral_path_host: fsnap_spectral_gram per problem from 16 Python threads);
  - the composed route that existed before: ONE fsnap_cv_candidates call per alpha with unit scales (64 calls; it factors
    every (fold, alpha) system and has NO rcond axis, so it covers a quarter of the grid);
  - numpy.linalg.eigh per problem from 16 threads (the eigendecompositions alone);
  - the layout, the statistics pass and the row pass of the per-class table, as the sister scripts time them;
on three sets of rows:
  - synth: 10^6 x 128 in 6 065 configurations of 30-300 rows;
  - ta:    the golden Ta rows, 15 213 x 31, blocks of 7 consecutive rows as configurations;
  - wide:  13 035 x 142 synthetic rows in 1 863 configurations of 7 rows;
each with the configurations dealt into F = 5 folds (folds5) and F = 40 (folds40).  Wall-clock times of the synchronous calls
(warm: after one call), median of --reps.  Every case is a child process under its own time limit; after one that did not end
well nothing more is started.

    python scripts/spectral_path_timing.py [--reps N] [--out FILE]
"""
import argparse
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from fitsnap_amd import _capi  # noqa: E402
from fitsnap_amd.solvers import folds as ff  # noqa: E402
from fitsnap_amd.solvers import spectral_path as sp  # noqa: E402
from bcs_path_timing import synth_rows, ta_rows, timed, wide_rows  # noqa: E402

FOLDS = {"folds5": 5, "folds40": 40}
CASES = [f"{rows}-{folds}" for rows in ("synth", "ta", "wide") for folds in FOLDS]
NCLASS, QA = 3, 64
RCONDS = np.array([0.0, 1e-7, 1e-5, 1e-3])
ROW_PASS_MAX = 4096                           # the row pass is timed while F * Q coefficient vectors stay at or below this


def case(name, reps, lines):
    which, fname = name.split("-")
    F = FOLDS[fname]
    A, b, w, sizes = {"synth": synth_rows, "ta": ta_rows, "wide": wide_rows}[which]()
    m, K = A.shape
    cfg = np.repeat(np.arange(len(sizes)), sizes)
    fold = np.random.default_rng(1).permutation(len(sizes))[cfg] % F
    nsub = NCLASS
    cat = (fold * nsub + (np.arange(m) % nsub)).astype(np.int32)
    ncat = F * nsub
    ctx = _capi.HipContext(0)
    ctx.upload_rows(A, b)
    ctx.set_weights(w)
    state = {}

    def prepare():
        state["layout"] = ctx.cat_prepare(cat, ncat)

    def stats():
        state["dptr"] = ctx.cat_normal_eq(state["layout"])
        ctx.download_packed(state["dptr"], K)              # the call only queues the kernels: wait for them (one block back)

    t_prep = timed(prepare, reps)
    t_stats = timed(stats, reps)
    blocks = ff.download_blocks(ctx, state["dptr"], ncat, K)
    folds, total = ff.sum_blocks(blocks, nsub)
    lmax = float(np.linalg.eigvalsh(ff.unpack(total, K)[0])[-1])
    alphas = np.concatenate([[0.0], lmax * np.logspace(-14, -1, QA - 1)])
    Q = QA * len(RCONDS)

    def device():
        state["dev"] = ctx.spectral_path(state["dptr"], K, F, nsub, alphas, RCONDS, False)
        state["ms"] = ctx.spectral_path_times()

    e1, e2 = [], []

    def device_events():
        device()
        e1.append(state["ms"][0])
        e2.append(state["ms"][1])

    t_dev = timed(device_events, reps)
    t_dev_coef = timed(lambda: ctx.spectral_path(state["dptr"], K, F, nsub, alphas, RCONDS, True), reps)
    t_host = timed(lambda: state.update(host=sp.spectral_path_host(blocks, K, alphas, RCONDS, nsub)), max(1, reps // 2))
    ones = np.ones((1, nsub))

    def composed():
        for a in alphas:
            ctx.cv_candidates(state["layout"], float(a), ones, F, K)

    try:
        t_comp = timed(composed, reps)
        comp = f"{t_comp:.2f} ms"
    except (ValueError, np.linalg.LinAlgError, _capi.FsnapError) as err:      # recorded plainly: the route refused the grid
        t_comp, comp = float("nan"), f"refused ({err})"
    systems = [ff.downdated(folds, total, f, K)[0] for f in range(F + 1)]

    def eigh_all():
        with ThreadPoolExecutor(max_workers=16) as pool:
            list(pool.map(np.linalg.eigh, systems))

    t_eigh = timed(eigh_all, reps)
    dev, hst = state["dev"], state["host"]
    same = all(np.array_equal(dev[i], hst[i]) for i in (0, 1, 2, 3, 4))
    lines.append(f"{name}: m = {m}, K = {K}, {len(sizes)} configurations, F = {F} folds, nsub = {nsub}: {F + 1} problems, Q = {Q} "
                 f"settings ({QA} alphas x {len(RCONDS)} rconds); Jacobi sweeps per problem {int(dev[2][:, 1].min())} ... "
                 f"{int(dev[2][:, 1].max())}, status {sorted(set(dev[2][:, 5].astype(int).tolist()))}")
    lines.append(f"  layout (fsnap_cat_prepare) {t_prep:.2f} ms   statistics pass C1 (fsnap_cat_normal_eq + one block back) {t_stats:.2f} ms")
    lines.append(f"  device route (fsnap_spectral_path, coef_out NULL) {t_dev:.2f} ms: kernel E1 {np.median(e1):.3f} ms, kernel E2 "
                 f"{np.median(e2):.3f} ms; with the {F * Q} coefficient vectors copied back {t_dev_coef:.2f} ms")
    lines.append(f"  host route (spectral_path_host: fsnap_spectral_gram from {min(ff.HOST_THREADS, os.cpu_count() or 1)} Python threads, "
                 f"without the download) {t_host:.2f} ms   numpy.linalg.eigh of the {F + 1} systems from 16 threads {t_eigh:.2f} ms")
    lines.append(f"  composed route before this entry point ({QA} fsnap_cv_candidates calls, unit scales, one per alpha; no rcond "
                 f"axis: {QA} of the {Q} settings) {comp}   device / composed {t_dev / t_comp:.3f}   device / host {t_dev / t_host:.3f}")
    lines.append(f"  eig, z, info, rank / dof / sse and fits device == host bit for bit: {same}")
    if F * Q <= ROW_PASS_MAX:
        full = ctx.spectral_path(state["dptr"], K, F, nsub, alphas, RCONDS, True)
        betas = np.ascontiguousarray(full[5].reshape(F * Q, K))
        t_rows = timed(lambda: ctx.candidate_rows(state["layout"], betas, None, _capi.CAND_ERROR_SUMS, ncat), max(1, reps // 2))
        lines.append(f"  row pass of the per-class table (fsnap_candidate_rows, {F * Q} vectors) {t_rows:.2f} ms")
    else:
        lines.append(f"  row pass of the per-class table: not timed, {F * Q} vectors are beyond this script's {ROW_PASS_MAX} "
                     f"(table='auto' takes the statistics table above folds.ROWS_TABLE_MAX = {ff.ROWS_TABLE_MAX})")
    ctx.close()


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
        r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--case-only", name, "--reps",
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
