"""Times of fsnap_ard_path (grouped K-fold ARD threshold paths, csrc/fsnap_ard.hip) on 10^6 x 128 rows in 6 065 configurations
of 30-300 rows, Q = 8 settings (logcut 0.3 ... 3), the configurations dealt into F = 5 folds (``folds5``) and F = 40 folds
(``groups40``):
  (a) the kernel call (fsnap_ard_path: upload of the hyper-parameters, kernels S1 and A1, download of the results);
  (b) the host route on the same downloaded blocks in the same process (ard_path.ard_path_host: ARD._ard_loop with pinvh from
      a pool of 16 Python threads);
  (c) what a user could do before this entry point existed: one ARD.perform_fit per (fold, setting) with the fold as the
      testing mask -- a fresh statistics pass, 5-20 host pinvh calls and as many passes over the rows for the residual.  It is
      timed over ONE fold x all Q settings and SCALED by F.
Also timed on their own: the layout (fsnap_cat_prepare), the statistics pass (fsnap_cat_normal_eq), the download of the blocks
and the row pass of the per-class table (fsnap_candidate_rows with F x Q vectors).  Wall-clock times of the synchronous calls,
warm (after one call), median of --reps.  Every case is a child process under its own time limit; after one that did not end
well nothing more is started.

    python scripts/ard_path_timing.py [--reps N] [--out FILE]
"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from fitsnap_amd.solvers import ard_path as ap  # noqa: E402
from fitsnap_amd.solvers import lasso_path as lp  # noqa: E402

CASES = {"folds5": 5, "groups40": 40}
LOGCUTS = [0.3, 0.6, 1.0, 1.3, 1.6, 2.0, 2.5, 3.0]
TOL, MAX_ITER, NCLASS = 1e-3, 1000, 3


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
    from fitsnap_amd import _capi
    from fitsnap_amd.config import Config
    from fitsnap_amd.parallel_tools import ParallelTools
    from fitsnap_amd.solvers import solver_factory

    F = CASES[name]
    A, b, w, sizes = rows()
    m, K = A.shape
    Q = len(LOGCUTS)
    cfg = np.repeat(np.arange(len(sizes)), sizes)
    fold = np.random.default_rng(1).permutation(len(sizes))[cfg] % F
    cat = (fold * NCLASS + (np.arange(m) % NCLASS)).astype(np.int32)
    ncat = F * NCLASS
    # the rows live in the shared arrays of a fitted ARD solver, as they do for a user; (a) and (b) run on its context
    pt = ParallelTools()
    for arr_name, arr in (("a", A), ("b", b), ("w", w)):
        pt.create_shared_array(arr_name, m, K if arr_name == "a" else 1)
        pt.shared_arrays[arr_name].array[:] = arr
    pt.fitsnap_dict.update({"Testing": [False] * m})

    def solver(logcut):
        return solver_factory.solver("ARD", pt, Config(pt, {"SOLVER": {"solver": "ARD"}, "ARD": {"logcut": logcut}}))

    pt.single_print = lambda *a, **k: None
    s = solver(LOGCUTS[0])
    s.perform_fit()
    ctx = pt.hip()
    state = {}

    def prepare():
        state["layout"] = ctx.cat_prepare(cat, ncat)

    def stats():
        state["dptr"] = ctx.cat_normal_eq(state["layout"])
        ctx.download_packed(state["dptr"], K)              # the call only queues the kernels: wait for them (one block back)

    def download():
        state["blocks"] = ap.download_blocks(ctx, state["dptr"], ncat, K)

    t_prep = timed(prepare, reps)
    t_stats = timed(stats, reps)
    t_down = timed(download, 1, warm=0)
    grid = [{"logcut": x, "scap": 1e-3, "scai": 1e-3} for x in LOGCUTS]
    hyper, run = ap.fold_hypers(*lp.sum_blocks(state["blocks"], NCLASS), K, grid, False)

    def device():
        state["dev"] = ctx.ard_path(state["dptr"], K, F, NCLASS, hyper, MAX_ITER, TOL)

    def host():
        state["host"] = ap.ard_path_host(state["blocks"], K, hyper, MAX_ITER, TOL, NCLASS)

    t_dev = timed(device, reps)
    t_dev1 = timed(lambda: ctx.ard_path(state["dptr"], K, F, NCLASS, np.ascontiguousarray(hyper[:, :1]), MAX_ITER, TOL), reps)
    t_host = timed(host, reps)
    coef, lam, info, held = state["dev"]
    hcoef, _, hinfo, _ = state["host"]
    same = bool(np.array_equal(info[:, :, [0, 1, 5]], hinfo[:, :, [0, 1, 5]]))
    diff = float(np.max(np.abs(coef - hcoef)) / np.max(np.abs(hcoef)))
    betas = np.ascontiguousarray(coef[:F].reshape(F * Q, K))
    t_rows = timed(lambda: ctx.candidate_rows(state["layout"], betas, None, _capi.CAND_ERROR_SUMS, ncat), reps)
    # (c): fold 0 as the testing mask, one perform_fit per setting
    pt.fitsnap_dict["Testing"] = (fold == 0).tolist()
    t_fits = []
    for logcut in LOGCUTS:
        sq = solver(logcut)
        t_fits.append(timed(sq.perform_fit, reps))
    t_base = float(np.sum(t_fits))
    lines.append(f"{name}: m = {m}, K = {K}, {len(sizes)} configurations, F = {F} folds, Q = {Q} (logcut {LOGCUTS[0]} ... {LOGCUTS[-1]}), "
                 f"nsub = {NCLASS}: {(F + 1) * Q} problems, tol = {TOL:g}, median of {reps}")
    lines.append(f"  layout (fsnap_cat_prepare) {t_prep:.2f} ms   statistics pass (fsnap_cat_normal_eq + one block back) {t_stats:.2f} ms   "
                 f"download of the {ncat} blocks {t_down:.2f} ms   row pass of the per-class table (fsnap_candidate_rows, {F * Q} vectors) "
                 f"{t_rows:.2f} ms")
    lines.append(f"  (a) device route (fsnap_ard_path) {t_dev:.2f} ms (Q = 1: {t_dev1:.2f} ms)   (b) host route (ard_path_host: _ard_loop from "
                 f"{min(lp.HOST_THREADS, os.cpu_count() or 1)} Python threads, without the download) {t_host:.2f} ms   (a) / (b) "
                 f"{t_dev / t_host:.3f}")
    lines.append(f"  (c) ARD.perform_fit with fold 0 as the testing mask, the {Q} settings one after the other: {t_base:.2f} ms "
                 f"({min(t_fits):.2f} ... {max(t_fits):.2f} ms each); SCALED by F = {F} (the all-rows fits not counted): "
                 f"{F * t_base:.2f} ms   (a) + layout + statistics against it: {(t_dev + t_prep + t_stats) / (F * t_base):.4f}")
    lines.append(f"  iterations per problem: median {int(np.median(info[:, :, 0]))}, {int(info[:, :, 0].min())} ... {int(info[:, :, 0].max())}; "
                 f"kept columns of the all-rows fits {int(info[F, :, 1].min())}-{int(info[F, :, 1].max())}; status other than 0: "
                 f"{int((info[:, :, 5] != 0).sum())}; iterations, kept counts and status equal to the host route's: {same}; largest "
                 f"difference device - host {diff:.1e} of the largest coefficient")
    pt.free()


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--case-only", default=None, choices=list(CASES))
    p.add_argument("--out", default=None)
    args = p.parse_args()
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
