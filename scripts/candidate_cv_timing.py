"""Timing of the grouped K-fold cross-validation of weight candidates (solvers/candidates_cv.py, kernels V0-V2 of
csrc/fsnap_cv.hip) against the composed route it replaces (fsnap_fit_candidates + fsnap_candidate_rows on the same
statistics).

    python scripts/candidate_cv_timing.py [--out profiles/candidate_cv_timing.txt]

ONE run: the driver starts one child process per shape, each under its own ``timeout -k 10``, one after the other, and stops
at the first child that fails.  Shapes: the golden Ta rows (15 213 x 31, its groups, configurations = blocks of 7 rows),
synthetic 13 035 x 142 (10 groups) and 10^6 x 128 in 6 065 configurations of 30 ... 300 rows, 40 groups x 3 row types; a
fifth of the configurations test; F = 5 folds; P = 32 and 128 seeded GA-style candidates.  Every figure is the median wall
time of --reps warm calls (host timers around synchronous calls, so launches, the copies of S, coefficients and sums and
the stream synchronisation are inside):
  stats_ms        fsnap_cat_normal_eq on the composite layout (F x C blocks) + a wait for the stream
  v1_ms           fsnap_cv_candidates (V0 + V1, P F problems)
  v2_ms           fsnap_cv_candidate_rows (V2 + C3R, ceil(P / 16) passes over the rows)
  device_ms       CandidateFits.cross_validate(method="device") on the held composite layout (V1 + V2 + pooling in numpy)
  composed_ms     CandidateFits.cross_validate(method="composed") on the same statistics
and at P = 16 on the same rows: v2_16_ms next to c3_16_ms = fsnap_candidate_rows(FSNAP_CAND_ERROR_SUMS) for 16 vectors, and
v2_fraction_of_8TBs = (categorised rows x K x 8 bytes) / v2_16_ms / 8 TB/s."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"15213x31": 240, "13035x142": 240, "1e6x128": 540}        # child time limits in seconds
F = 5


def candidates(groups, P, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(P):
        ew = 10.0 ** rng.uniform(-4, 4, len(groups))
        fr = 10.0 ** rng.uniform(-3, 3, len(groups))
        sr = 10.0 ** rng.uniform(-3, 3, len(groups))
        out.append({g: {"eweight": ew[i], "fweight": ew[i] * fr[i], "vweight": ew[i] * sr[i]} for i, g in enumerate(groups)})
    return out


def rows_of(name):
    if name == "15213x31":
        z = np.load(os.path.join(ROOT, "tests", "golden", "ta_abw.npz"))
        f = np.load(os.path.join(ROOT, "tests", "golden", "ta_reference_fits.npz"))
        m = len(z["b"])
        fs = {"Groups": np.asarray(f["ea_groups"]).astype(str), "Testing": np.asarray(f["testing_mask"], dtype=bool),
              "Row_Type": np.array(["Energy"] * 363 + ["Force"] * 12672 + ["Stress"] * 2178),
              "Configs": np.char.add("c", (np.arange(m) // 7).astype(str))}
        return np.ascontiguousarray(z["A"]), np.ascontiguousarray(z["b"]), fs
    r = np.random.default_rng(1)
    if name == "13035x142":
        K, ng, sizes = 142, 10, np.full(13_035 // 15, 15)
    else:
        K, ng, sizes = 128, 40, r.integers(30, 301, 6065)
    m = int(sizes.sum())
    cfg = np.repeat(np.arange(len(sizes)), sizes)
    first = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    pos = np.arange(m) - np.repeat(first, sizes)
    rt = np.where(pos == 0, "Energy", np.where(pos >= np.repeat(sizes, sizes) - 6, "Stress", "Force"))
    A = r.standard_normal((m, K)) * np.exp(0.5 * r.standard_normal(K))
    b = A @ r.standard_normal(K) + 0.05 * r.standard_normal(m)
    g = np.repeat(r.integers(0, ng, len(sizes)), sizes)
    fs = {"Groups": np.char.add("g", np.char.zfill(g.astype(str), 2)), "Testing": np.repeat(r.random(len(sizes)) < 0.2, sizes),
          "Row_Type": rt, "Configs": np.char.add("c", cfg.astype(str))}
    return A, b, fs


def median_ms(f, reps):
    f()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        t.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(t))


def child(name, reps):
    from fitsnap_amd import _capi
    from fitsnap_amd.config import Config
    from fitsnap_amd.parallel_tools import ParallelTools
    from fitsnap_amd.solvers import CandidateFits, solver_factory
    from fitsnap_amd.solvers import candidates_cv as ccv

    A, b, fs = rows_of(name)
    pt = ParallelTools()
    s = solver_factory.solver("SVD", pt, Config(pt, {"SOLVER": {"solver": "SVD"}}))
    cf = CandidateFits(s, A, b, fs_dict=fs)
    groups = sorted(set(fs["Groups"]))
    K, C = cf.K, cf.ncat
    S16 = cf.scales_from_group_weights(candidates(groups, 16, 4))
    t0 = time.perf_counter()
    cv = cf.cross_validate(S16, folds=F, by="Configs")                    # prepares the composite layout and its statistics
    setup = time.perf_counter() - t0
    ctx, tag = pt.hip(), cf._cv[0]
    rows = int(np.count_nonzero(cf._cv[1] >= 0))
    one = np.empty(1)

    def stats():
        ctx.dev_download(ctx.cat_normal_eq(tag), one)

    out = {"shape": name, "K": K, "C": C, "F": F, "categorised_rows": rows, "setup_s": setup, "stats_ms": median_ms(stats, reps)}
    v2 = median_ms(lambda: ctx.cv_candidate_rows(tag, cv.coef, C), reps)
    c3 = median_ms(lambda: ctx.candidate_rows(tag, cv.coef[:, 0], None, _capi.CAND_ERROR_SUMS, F * C), reps)
    out.update(v2_16_ms=v2, c3_16_ms=c3, v2_fraction_of_8TBs=rows * K * 8 / (v2 * 1e-3) / 8e12,
               c3_fraction_of_8TBs=rows * K * 8 / (c3 * 1e-3) / 8e12)
    print(json.dumps(out), flush=True)
    for P in (32, 128):
        S = cf.scales_from_group_weights(candidates(groups, P, 5))
        coef, info = ctx.cv_candidates(tag, 0.0, S, F, K)
        rec = {"shape": name, "P": P, "problems": P * F, "failed": int(info[:, :, 0].sum()),
               "v1_ms": median_ms(lambda: ctx.cv_candidates(tag, 0.0, S, F, K), reps),
               "v2_ms": median_ms(lambda: ctx.cv_candidate_rows(tag, coef, C), reps),
               "device_ms": median_ms(lambda: cf.cross_validate(S, folds=F, by="Configs", method="device"), reps),
               "composed_ms": median_ms(lambda: cf.cross_validate(S, folds=F, by="Configs", method="composed"), max(2, reps // 3))}
        rec["v1_ms_per_problem"] = rec["v1_ms"] / (P * F)
        rec["composed_over_device"] = rec["composed_ms"] / rec["device_ms"]
        dev = cf.cross_validate(S, folds=F, by="Configs", method="device")
        comp = cf.cross_validate(S, folds=F, by="Configs", method="composed")
        ok = ~(dev.status.any(axis=1) | comp.status.any(axis=1))
        a, c = dev.row_type_errors[ok, :, 1], comp.row_type_errors[ok, :, 1]
        rec["max_rel_rmse_device_vs_composed"] = float(np.max(np.abs(a - c) / c)) if ok.any() else None
        print(json.dumps(rec), flush=True)
    assert cf._cv[0] == tag                                              # every timed call ran on the same statistics
    pt.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--shape", default=None, help="run one shape in this process (what the driver starts)")
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    args = ap.parse_args()
    if args.shape:
        child(args.shape, args.reps)
        return 0
    lines = ["# scripts/candidate_cv_timing.py on one MI355X (gfx950): medians of warm calls, wall ms, one run"]
    for name, limit in SHAPES.items():
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--shape", name,
                            "--reps", str(args.reps)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        got = [l for l in r.stdout.splitlines() if l.startswith("{")]
        print("\n".join(got), flush=True)
        lines += got
        if r.returncode != 0:                                            # a failure ends the run: nothing more is started
            print(f"{name}: exit {r.returncode}\n{r.stderr[-2000:]}", file=sys.stderr)
            return r.returncode
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
