"""Accuracy record of the joint unit scores (profiles/select_joint_accuracy.txt): on the kernel cases of
tests/select_joint_cases.py (K = 31, 64, 128, 142, 160; units of 1 ... 300 rows; J = K and J = K - 5) the worst error against
the long-double evaluation of the kernel's formulas of (a) the float64 numpy mirror (select_joint.unit_scores_host; needs no
GPU) and, when a GPU is present, (b) kernels J1 / J2 -- relative, and in units of the rounding bound derived from the term
counts (select_joint_cases.long_double_scores).

    python scripts/select_joint_accuracy.py [--out FILE]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import select_joint_cases as jc  # noqa: E402
from fitsnap_amd import _capi  # noqa: E402
from fitsnap_amd.solvers import select_joint as sj  # noqa: E402


def worst(got, ref, live):
    out = []
    for i, crit in enumerate(sj.CRITERIA):
        err = np.abs(got[crit][live] - ref[i][live])
        nz = ref[i][live] != 0
        out.append((float(np.max(err[nz] / np.abs(ref[i][live][nz]))), float(np.max(err / np.maximum(ref[2 + i][live], 1e-300)))))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    gpu = _capi.device_count() > 0
    lines = ["case: worst error against long double as (relative, share of the term-count bound), gain | reduction"]
    top = {"mirror": [[0, 0], [0, 0]], "kernel": [[0, 0], [0, 0]]}
    for K in jc.KERNEL_KS:
        p = jc.kernel_case(K)
        for J, r, tau in ((K, K, p["tau"]), (K - 5, K - 3, 3.0 * p["tau"])):
            q = dict(p, M=np.ascontiguousarray(p["M"][:, :J]), B=np.ascontiguousarray(p["B"][:J, :r]), tau=tau)
            ref = jc.long_double_case(q)
            live = p["sizes"] > 0
            runs = {}
            rows, off = sj.unit_layout(p["cat"], p["ncat"])
            A = np.ascontiguousarray(p["A"])
            runs["mirror"] = {"gain": np.full(p["ncat"], np.nan), "reduction": np.full(p["ncat"], np.nan)}
            for u in np.flatnonzero(live):
                sel = rows[off[u]:off[u + 1]]
                g, rd, _, _ = sj.score_one(p["w"][sel, None] * A[sel], q["M"], tau, q["B"])
                runs["mirror"]["gain"][u], runs["mirror"]["reduction"][u] = g, rd
            if gpu:
                ctx = _capi.HipContext(0)
                ctx.upload_rows(p["A"], np.zeros(A.shape[0]))
                ctx.joint_begin(rows, off, p["w"])
                runs["kernel"] = ctx.joint_score(q["M"], tau, q["B"])
                ctx.close()
            for name, got in runs.items():
                wv = worst(got, ref, live)
                lines.append(f"K={K:3d} J={J:3d} r={r:3d} {name}: ({wv[0][0]:.2e}, {wv[0][1]:.2e}) | ({wv[1][0]:.2e}, {wv[1][1]:.2e})")
                for i in range(2):
                    for j in range(2):
                        top[name][i][j] = max(top[name][i][j], wv[i][j])
    for name in ("mirror", "kernel") if gpu else ("mirror",):
        t = top[name]
        lines.append(f"worst over all cases, {name}: gain ({t[0][0]:.2e}, {t[0][1]:.2e}) | reduction ({t[1][0]:.2e}, {t[1][1]:.2e})")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
