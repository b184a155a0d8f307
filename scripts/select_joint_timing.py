"""Times of the joint unit scores (fsnap_joint_score, csrc/fsnap_joint.hip; Solver.select_units) at the shape of
profiles/loco_timing.txt: 10^6 x 128 pool rows in 6 065 units of 30-300 rows, posterior factor M (128 x 128), target = the
pool itself (r = 128).
  - fsnap_joint_score call for the gain alone and for gain + reduction: wall time of the synchronous library call (warm:
    after two calls), median of --reps;
  - Solver.select_units per pick (score call + host factor of C + downdate), --picks picks per criterion;
  - select_joint.unit_scores_host (numpy, the BLAS pool as it is) on the first --host-units units, scaled to all units.
Kernel times (J1 fsnap_joint_rows_k, J2 fsnap_joint_unit_k<D>) come from a run of its own under
rocprofv3 --kernel-trace --stats with --kernels-only.

    python scripts/select_joint_timing.py [--reps N] [--picks P] [--host-units U] [--kernels-only] [--out FILE]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from fitsnap_amd import _capi  # noqa: E402
from fitsnap_amd.config import Config  # noqa: E402
from fitsnap_amd.parallel_tools import ParallelTools  # noqa: E402
from fitsnap_amd.solvers import select_joint as sj, solver_factory  # noqa: E402


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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--picks", type=int, default=4)
    ap.add_argument("--host-units", type=int, default=120)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []
    K = 128
    rng = np.random.default_rng(0)
    sizes = rng.integers(30, 301, 7000)
    sizes = sizes[:int(np.searchsorted(np.cumsum(sizes), 1_000_000)) + 1]     # the units of scripts/loco_timing.py
    m, nu = int(sizes.sum()), len(sizes)
    A = rng.standard_normal((m, K))
    w = rng.uniform(0.5, 2.0, m)
    cat = np.repeat(np.arange(nu), sizes).astype(np.int32)
    At = rng.standard_normal((20000, K))
    tau = 0.04
    C0 = tau * np.linalg.inv(At.T @ At + 1e-8 * np.eye(K))
    C0 = 0.5 * (C0 + C0.T)
    M = sj.factor_cov(C0)
    ctx = _capi.HipContext(0)
    ctx.upload_rows(A, np.zeros(m))
    ctx.set_weights(np.ones(m))
    T = ctx.normal_eq()[0]
    B = M.T @ sj.target_factor(T).T
    rows, off = sj.unit_layout(cat, nu)
    ctx.joint_begin(rows, off, w)
    if args.kernels_only:
        for _ in range(3):
            ctx.joint_score(M, tau)
        for _ in range(3):
            ctx.joint_score(M, tau, B)
        ctx.close()
        return
    t_gain = timed(lambda: ctx.joint_score(M, tau), args.reps)
    t_both = timed(lambda: ctx.joint_score(M, tau, B), args.reps)
    t_red = timed(lambda: ctx.joint_score(M, tau, B, want_gain=False), args.reps)
    res = ctx.joint_score(M, tau, B)
    d = res["info"][:, 0]
    bins = [int((d <= 32).sum()), int(((d > 32) & (d <= 64)).sum()), int(((d > 64) & (d <= 128)).sum()), int((d > 128).sum())]
    lines.append(f"m = {m}, K = {K}, J = {M.shape[1]}, r = {B.shape[1]}, {nu} units of {sizes.min()}-{sizes.max()} rows; dim S bins "
                 f"<=32 / <=64 / <=128 / general: {bins}; n space {int(res['info'][:, 1].sum())}")
    lines.append(f"  fsnap_joint_score call, gain alone        {t_gain:8.3f} ms")
    lines.append(f"  fsnap_joint_score call, reduction alone   {t_red:8.3f} ms")
    lines.append(f"  fsnap_joint_score call, gain + reduction  {t_both:8.3f} ms")
    # the host mirror on the first units, scaled
    hu = min(args.host_units, nu)
    sub = cat < hu
    Ah, ch, wh = np.ascontiguousarray(A[sub]), cat[sub], w[sub]
    for crit in sj.CRITERIA:
        t0 = time.perf_counter()
        h = sj.unit_scores_host(Ah, ch, hu, None, wh, tau, T, (crit,), M=M)
        th = time.perf_counter() - t0
        err = np.max(np.abs(h[crit] - res[crit][:hu]) / np.abs(h[crit]))
        lines.append(f"  unit_scores_host, {crit}: {1e3 * th:.1f} ms for {hu} units -> {th * nu / hu:.2f} s for all {nu} "
                     f"(GPU against it: {err:.1e} relative)")
    ctx.close()
    # Solver.select_units per pick
    pt = ParallelTools()
    sol = solver_factory.solver("ANL", pt, Config(pt, {"SOLVER": {"solver": "ANL"}}))
    sol.cov = C0
    for crit in sj.CRITERIA:
        kw = dict(a=A, w=w, categories=cat, criterion=crit, noise=tau)
        sol.select_units(0, **kw)
        t0 = time.perf_counter()
        sol.select_units(0, **kw)
        t_zero = time.perf_counter() - t0
        t0 = time.perf_counter()
        sol.select_units(args.picks, **kw)
        t_p = time.perf_counter() - t0
        lines.append(f"  Solver.select_units, {crit}: {1e3 * (t_p - t_zero) / args.picks:.2f} ms per pick ({args.picks} picks; a call "
                     f"with 0 picks, one scoring included: {1e3 * t_zero:.1f} ms)")
    pt.free()
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
