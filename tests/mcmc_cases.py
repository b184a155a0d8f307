"""Shared by the MCMC tests: the golden cases of tests/golden/ta_mcmc_reference.npz (from the reference's own MCMC class,
see make_golden_mcmc.py) and a numpy restatement of the reference's log-posterior as a chain evaluator."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_golden():
    return np.load(os.path.join(GOLDEN, "ta_mcmc_reference.npz"))


def case_rows(g, tag):
    """(aw, bw) the reference's chain runs on for golden case ``tag`` (mcmc.py:100-118): the weighted training rows, or
    (aw^T aw, aw^T bw) with apply_transpose."""
    z = np.load(os.path.join(GOLDEN, "ta_abw.npz"))
    train = ~g[f"{tag}_testing"]
    w = z["w"][train]
    aw, bw = w[:, None] * z["A"][train], w * z["b"][train]
    if int(g[f"{tag}_transpose"]):
        return aw.T @ aw, aw.T @ bw
    return aw, bw


def numpy_evaluator(aw, bw, sigma, calls=None):
    """-logpost of every row of U, each with the reference's own expression (mcmc.py:80-88)."""
    s2 = sigma * sigma
    norm_const = -0.5 * np.log(2 * np.pi * s2)

    def evaluate(U):
        if calls is not None:
            calls.append(len(U))
        out = np.empty(len(U))
        for i, x in enumerate(U):
            x_mu = aw @ x - bw
            out[i] = -np.sum(norm_const - 0.5 * x_mu * x_mu / s2)
        return out

    return evaluate


def relmax(x, ref):
    x, ref = np.asarray(x), np.asarray(ref)
    return float(np.max(np.abs(x - ref)) / max(np.max(np.abs(ref)), 1e-300))
