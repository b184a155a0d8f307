"""Timing of the MCMC pass (fsnap_sse_batch, kernel S1 / S1G) next to kernel C3 on the same work, and of whole chains.

    python scripts/mcmc_timing.py --calls           # call wall times (and the traced launches of the kernel-trace run)
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o mcmc -- python scripts/mcmc_timing.py --calls
    python scripts/mcmc_timing.py --kernel-trace <dir>/mcmc_kernel_trace.csv      # kernel times -> share of 8 TB/s
    python scripts/mcmc_timing.py --chains          # 10 000-step chains: SPECULATE 16 and 1, and a numpy amcmc

--calls: at 10^6 x 128 (synthetic) fsnap_sse_batch with P = 1 and P = 16, then kernel C3 (fsnap_candidate_rows, error sums,
one category holding every row) with the same 16 vectors and with 1; then fsnap_sse_batch with P = 16 at 15 213 x 31 (the
golden Ta rows) and 13 035 x 142 (synthetic).  One pass moves 8K + 17 bytes per row (the row, b, w, the mask byte).  Kernel
time per call = the row kernel plus its fold, median over the timed calls.
--chains: MCMC.perform_fit with mcmc_num = 10 000 (gamma 0.01, sigma 0.1) on the Ta rows and on synthetic 10^6 x 128 rows,
a warm-up fit and then the timed one; wall time, passes and steps per pass.  The numpy restatement runs the same chain
(run_chain with the reference's log-posterior expression, one proposal per evaluation) with 16 BLAS threads: in full on
the Ta rows, and at 10^6 x 128 as the measured time of one numpy evaluation times the number of evaluations."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from fitsnap_amd import _capi  # noqa: E402

HBM = 8.0e12
WARMUP, REPS = 5, 50


def synth(m, K, seed=1):
    r = np.random.default_rng(seed)
    A = r.standard_normal((m, K)) * np.exp(0.5 * r.standard_normal(K))
    b = A @ r.standard_normal(K) + 0.05 * r.standard_normal(m)
    return A, b, 0.5 + r.random(m)


def ta():
    z = np.load(os.path.join(ROOT, "tests", "golden", "ta_abw.npz"))
    return np.ascontiguousarray(z["A"]), np.ascontiguousarray(z["b"]), np.ascontiguousarray(z["w"])


def timed(fn):
    for _ in range(WARMUP):
        fn()
    t = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return float(np.median(t))


# (label, shape, kernel-name fragment) in the order --calls launches them
CALLS = [("sse P=1", "1e6x128", "fsnap_sse_rows_k"), ("sse P=16", "1e6x128", "fsnap_sse_rows_k"),
         ("C3 P=16", "1e6x128", "fsnap_cand_rows_k"), ("C3 P=1", "1e6x128", "fsnap_cand_rows_k"),
         ("sse P=16", "15213x31", "fsnap_sse_rows_k"), ("sse P=16", "13035x142", "fsnap_sse_rows_k")]
SHAPES = {"1e6x128": (1_000_000, 128), "15213x31": (15_213, 31), "13035x142": (13_035, 142)}


def calls():
    r = np.random.default_rng(2)
    A, b, w = synth(1_000_000, 128)
    ctx = _capi.HipContext(0)
    ctx.upload_rows(A, b)
    ctx.set_weights(w)
    U = r.standard_normal((16, 128))
    out = []
    out.append(("sse P=1", "1e6x128", timed(lambda: ctx.sse_batch(U[:1]))))
    out.append(("sse P=16", "1e6x128", timed(lambda: ctx.sse_batch(U))))
    tag = ctx.cat_prepare(np.zeros(A.shape[0], dtype=np.int32), 1)
    out.append(("C3 P=16", "1e6x128", timed(lambda: ctx.candidate_rows(tag, U, None, _capi.CAND_ERROR_SUMS, 1))))
    out.append(("C3 P=1", "1e6x128", timed(lambda: ctx.candidate_rows(tag, U[:1], None, _capi.CAND_ERROR_SUMS, 1))))
    ctx.close()
    for name, (A, b, w) in (("15213x31", ta()), ("13035x142", synth(13_035, 142))):
        ctx = _capi.HipContext(0)
        ctx.upload_rows(A, b)
        ctx.set_weights(w)
        U = r.standard_normal((16, A.shape[1]))
        out.append(("sse P=16", name, timed(lambda: ctx.sse_batch(U))))
        ctx.close()
    for label, shape, t in out:
        m, K = SHAPES[shape]
        print(json.dumps({"call": label, "shape": shape, "call_wall_ms_median": t * 1e3,
                          "hbm_share_at_wall": m * (8 * K + 17) / t / HBM}), flush=True)


def kernel_trace(path):
    import csv

    rows = [r for r in csv.DictReader(open(path))
            if any(k in r["Kernel_Name"] for k in ("fsnap_sse_rows_k", "fsnap_cand_", "fsnap_colsum"))]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    # a call = the row kernel and everything after it up to the next row kernel (its fold / reductions)
    per_call, cur = [], None
    for r in rows:
        dt = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-9
        row_kernel = "fsnap_sse_rows_k" in r["Kernel_Name"] or "fsnap_cand_rows_k" in r["Kernel_Name"]
        if row_kernel:
            if cur is not None:
                per_call.append(cur)
            cur = [r["Kernel_Name"], dt, dt]
        elif cur is not None:
            cur[2] += dt
    if cur is not None:
        per_call.append(cur)
    per = WARMUP + REPS
    for i, (label, shape, frag) in enumerate(CALLS):
        block = per_call[i * per:(i + 1) * per][WARMUP:]
        assert all(frag in c[0] for c in block), (label, {c[0] for c in block})
        row_t = float(np.median([c[1] for c in block]))
        tot_t = float(np.median([c[2] for c in block]))
        m, K = SHAPES[shape]
        nbytes = m * (8 * K + 17)
        print(json.dumps({"call": label, "shape": shape, "row_kernel_ms": row_t * 1e3, "with_fold_ms": tot_t * 1e3,
                          "bytes": nbytes, "hbm_share_row_kernel": nbytes / row_t / HBM,
                          "hbm_share_with_fold": nbytes / tot_t / HBM}))


def chains():
    from fitsnap_amd.config import Config
    from fitsnap_amd.parallel_tools import ParallelTools
    from fitsnap_amd.solvers import mcmc as mcmc_mod
    from fitsnap_amd.solvers import solver_factory
    from fitsnap_amd._hostblas import blas_threads

    nmcmc = 10_000
    for name, (A, b, w) in (("Ta 15213x31", ta()), ("synthetic 1e6x128", synth(1_000_000, 128))):
        w = w * (10.0 if A.shape[0] > 100_000 else 1.0)      # synthetic: acceptance after the warm-up near the Ta chain's
        for spec in (16, 1):
            mcmc_mod.SPECULATE = spec
            pt = ParallelTools()
            cfg = Config(pt, {"SOLVER": {"solver": "MCMC", "mcmc_num": nmcmc, "mcmc_gamma": 0.01, "mcmc_sigma": 0.1}})
            s = solver_factory.solver("MCMC", pt, cfg)
            s.save_files = False
            for _ in range(2):                                # warm-up fit, then the timed one
                np.random.seed(0)
                t0 = time.perf_counter()
                s.perform_fit(A, b, w, trainall=True)
                t = time.perf_counter() - t0
            steps = nmcmc - 1
            print(json.dumps({"chain": name, "speculate": spec, "steps": steps, "wall_s": t, "passes": s.passes,
                              "steps_per_pass": steps / s.passes, "acc_rate": s.acc_rate}), flush=True)
            start, acc = s.samples[0].copy(), s.accepted.copy()
            pt.free()
        mcmc_mod.SPECULATE = 16
        aw, bw = w[:, None] * A, w * b
        s2 = 0.1 * 0.1
        nc = -0.5 * np.log(2 * np.pi * s2)
        count = [0]

        def evaluate(U):
            count[0] += len(U)
            out = np.empty(len(U))
            for i, x in enumerate(U):
                x_mu = aw @ x - bw
                out[i] = -np.sum(nc - 0.5 * x_mu * x_mu / s2)
            return out

        with blas_threads(16):
            if A.shape[0] < 100_000:
                np.random.seed(0)
                t0 = time.perf_counter()
                res = mcmc_mod.run_chain(start, nmcmc, 0.01, evaluate, speculate=1)
                t = time.perf_counter() - t0
                print(json.dumps({"chain": name, "numpy_amcmc_16_threads_wall_s": t, "evaluations": count[0],
                                  "same_accept_pattern": bool(np.array_equal(res.accepted, acc))}), flush=True)
            else:
                x = start[None, :]
                te = timed(lambda: evaluate(x))
                nev = 1 + int(np.count_nonzero(np.arange(steps) >= 200))
                print(json.dumps({"chain": name, "numpy_evaluation_ms": te * 1e3, "evaluations_of_the_chain": nev,
                                  "numpy_amcmc_16_threads_estimated_s": te * nev}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", action="store_true")
    ap.add_argument("--chains", action="store_true")
    ap.add_argument("--kernel-trace")
    args = ap.parse_args()
    if args.kernel_trace:
        kernel_trace(args.kernel_trace)
    if args.calls:
        calls()
    if args.chains:
        chains()


if __name__ == "__main__":
    main()
