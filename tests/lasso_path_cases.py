"""Cases, oracles and tolerances of the grouped K-fold LASSO alpha path (tests/test_lasso_path_cpu.py,
tests/test_gpu_lasso_path.py).

Oracle A: ``lasso_path.lasso_path_host`` -- ``_capi.lasso_gram`` on the fold blocks downdated in numpy (the same subtraction
and summation order as the kernel).  Oracle B: scikit-learn's ``Lasso(alpha, fit_intercept=False, tol=1e-13,
max_iter=200000)`` on the weighted rows without the fold (what the reference's class calls).

Acceptance of coefficients (no sweep-count equality: FMA contraction may move a stopping test by one sweep):
  1. ``check_gap``: the duality gap of the RETURNED coefficients, recomputed in long double, is below tol y2 (1 + 1e-9)
     whenever sweeps < max_iter, and the reported gap agrees with it to 1e-6 relative or 64 K eps y2 absolute.
  2. ``bound2``: with lambda the smallest eigenvalue of the live part of Qm the objective is lambda-strongly convex, so
     ||beta - beta_oracle||_2 <= sqrt(2 gap / lambda) + sqrt(2 gap_oracle / lambda) + 64 K eps ||beta||_2.
  3. ``TIGHT_REL`` at tol = 1e-12 against oracle A, and ``HELDOUT_REL`` for the held-out sums: 10 x what the plain float64
     restatements below differ by on the sweep's cases (measured by ``python tests/lasso_path_cases.py``, recorded here).
"""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from fitsnap_amd.solvers import lasso_path as lp  # noqa: E402

LD = np.longdouble
EPS = np.finfo(np.float64).eps

SWEEP_K = [1, 7, 31, 63, 64, 65, 128, 129, 143, 144]     # lane-ownership edges of a 64-lane wave, the LDS-size edge
SWEEP_F, SWEEP_Q = 3, 4
GRID4 = np.array([0.5, 0.05, 1e-3, 1e-5])                # fractions of max |c| / n
GRID8 = np.array([0.5, 0.1, 0.02, 5e-3, 1e-3, 2e-4, 5e-5, 1e-5])
TIGHT_TOL = 1e-12
MAX_ITER = 100000

# Measured on the sweep's cases (SWEEP_K x (F + 1) x Q problems, tol = 1e-12) by ``python tests/lasso_path_cases.py``:
#   plain Python float64 restatement of the iteration (cd_numpy) against oracle A, relative ||.||_2:  worst MEASURED_TIGHT
#   numpy float64 three-term held-out formula against the row-wise long-double sum, relative:          worst MEASURED_HELDOUT
# The kernel is allowed 10 x each (FMA contraction, reduction order).
MEASURED_TIGHT = 3.8e-15
MEASURED_HELDOUT = 4.0e-12
TIGHT_REL = 10 * MEASURED_TIGHT
HELDOUT_REL = 10 * MEASURED_HELDOUT


def fold_rows(seed, K, fold_sizes, nclass=3, nonzero_frac=0.4, noise=0.1):
    """Rows with columns scaled over two decades, a sparse truth and weights in [0.5, 2]: (A, b, w, fold id per row, class per
    row).  The folds are contiguous blocks of ``fold_sizes`` rows."""
    rng = np.random.default_rng(seed)
    m = int(sum(fold_sizes))
    scale = 10.0 ** rng.uniform(-1.0, 1.0, K)
    A = rng.standard_normal((m, K)) * scale
    truth = np.where(rng.random(K) < nonzero_frac, rng.standard_normal(K), 0.0) / scale
    if K and not truth.any():
        truth[0] = 1.0 / scale[0]
    b = A @ truth + noise * rng.standard_normal(m)
    w = rng.uniform(0.5, 2.0, m)
    fold = np.repeat(np.arange(len(fold_sizes)), fold_sizes).astype(np.int64)
    cls = (np.arange(m) % nclass).astype(np.uint8)
    return A, b, w, fold, cls


@functools.lru_cache(maxsize=None)
def sweep_case(K):
    """The geometry sweep's rows at K: F = 3 folds of about 3 K + 40 rows."""
    return fold_rows(4000 + K, K, [3 * K + 40, 3 * K + 41, 3 * K + 39])


def blocks_numpy(A, b, w, cat, ncat):
    """The packed per-category blocks [G | c | bb, sum wb, n] in numpy float64 (what fsnap_cat_normal_eq forms on the GPU, to
    rounding): ncat x (K^2 + K + 3).  cat < 0: the row takes no part."""
    K = A.shape[1]
    out = np.zeros((ncat, K * K + K + 3))
    for c in range(ncat):
        r = np.flatnonzero(cat == c)
        X, y = A[r] * w[r, None], b[r] * w[r]
        out[c, :K * K] = (X.T @ X).ravel()
        out[c, K * K:K * K + K] = X.T @ y
        out[c, K * K + K:] = (y @ y, y.sum(), len(r))
    return out


def alpha_grid(blocks, K, fractions, nsub=1):
    """alphas = fractions x max |c| / n of the total: the first leaves a handful of coefficients, the last nearly all."""
    _, total = lp.sum_blocks(blocks, nsub)
    _, c, _, n = lp.unpack(total, K)
    return np.asarray(fractions, dtype=np.float64) * float(np.max(np.abs(c))) / n


def cd_numpy(Qm, qv, y2, l1, max_iter, tol):
    """fsnap_lasso_gram restated in plain Python float64 (no FMA): (w, sweeps, gap)."""
    K = len(qv)
    w, H = np.zeros(K), np.zeros(K)
    gap_tol = tol * y2
    gap = gap_tol + 1.0
    it = 0
    while it < max_iter:
        w_max = d_w_max = 0.0
        for i in range(K):
            Qii = Qm[i, i]
            if Qii == 0.0:
                continue
            w_old = w[i]
            if w_old != 0.0:
                H -= w_old * Qm[i]
            t = qv[i] - H[i]
            mag = abs(t) - l1
            w_new = float(np.copysign(mag, t)) / Qii if mag > 0.0 else 0.0
            w[i] = w_new
            if w_new != 0.0:
                H += w_new * Qm[i]
            d_w_max = max(d_w_max, abs(w_new - w_old))
            w_max = max(w_max, abs(w_new))
        if w_max == 0.0 or d_w_max / w_max < tol or it == max_iter - 1:
            qdw, wHw, l1n = float(w @ qv), float(w @ H), float(np.abs(w).sum())
            dual = float(np.max(np.abs(qv - H))) if K else 0.0
            r2 = y2 + wHw - 2.0 * qdw
            if dual > l1:
                c = l1 / dual
                gap = 0.5 * (r2 + r2 * c * c)
            else:
                c, gap = 1.0, r2
            gap += l1 * l1n - c * y2 + c * qdw
            if gap < gap_tol:
                it += 1
                break
        it += 1
    return w, min(it, max_iter), gap


def gap_ld(Qm, qv, y2, l1, beta):
    """The duality gap of ``beta`` for (1/2) w^T Qm w - qv^T w + l1 |w|_1 (+ y2 / 2) in long double, as fsnap_lasso_gram
    defines it."""
    Q, q, w = np.asarray(Qm, dtype=LD), np.asarray(qv, dtype=LD), np.asarray(beta, dtype=LD)
    y2, l1 = LD(y2), LD(l1)
    H = Q @ w
    qdw, wHw, l1n = w @ q, w @ H, np.abs(w).sum()
    dual = np.max(np.abs(q - H)) if len(w) else LD(0)
    r2 = y2 + wHw - 2 * qdw
    if dual > l1:
        c = l1 / dual
        gap = (r2 + r2 * c * c) / 2
    else:
        c, gap = LD(1), r2
    return gap + l1 * l1n - c * y2 + c * qdw


def check_gap(Qm, qv, y2, l1, beta, sweeps, reported, max_iter, tol, where=""):
    """Acceptance 1."""
    K = len(qv)
    true = float(gap_ld(Qm, qv, y2, l1, beta))
    if sweeps < max_iter:
        assert true < tol * y2 * (1 + 1e-9), (where, "gap", true, "tol y2", tol * y2, "sweeps", sweeps)
    assert abs(reported - true) <= max(1e-6 * abs(true), 64 * K * EPS * y2), (where, "reported", reported, "true", true)
    return true


def bound2(Qm, dead, gap, gap_oracle, beta):
    """Acceptance 2's bound on ||beta - beta_oracle||_2 (inf when the live part of Qm is not positive definite)."""
    live = ~np.asarray(dead, dtype=bool)
    K = len(beta)
    if not live.any():
        return 64 * K * EPS * float(np.linalg.norm(beta))
    lam = float(np.linalg.eigvalsh(Qm[np.ix_(live, live)])[0])
    if lam <= 0:
        return np.inf
    return (np.sqrt(2 * max(gap, 0.0) / lam) + np.sqrt(2 * max(gap_oracle, 0.0) / lam)
            + 64 * K * EPS * float(np.linalg.norm(beta)))


def sklearn_refit(A, b, w, train, alpha):
    """Oracle B on the weighted rows ``train`` (boolean mask): the coefficients."""
    from sklearn.linear_model import Lasso

    import warnings

    X, y = A[train] * w[train, None], b[train] * w[train]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        if alpha == 0.0:                                  # scikit-learn advises against alpha = 0: the normal equations
            return np.linalg.lstsq(X, y, rcond=None)[0]
        return Lasso(alpha=float(alpha), fit_intercept=False, tol=1e-13, max_iter=200000).fit(X, y).coef_.copy()


def heldout_ld(A, b, w, rows, beta):
    """sum (w (b - a . beta))^2 over ``rows`` in long double."""
    r = (np.asarray(b[rows], dtype=LD) - np.asarray(A[rows], dtype=LD) @ np.asarray(beta, dtype=LD)) * np.asarray(w[rows], dtype=LD)
    return float(r @ r)


def heldout_numpy(block, K, beta):
    """The three-term formula in numpy float64."""
    G, c, bb, _ = lp.unpack(block, K)
    return bb - 2.0 * (beta @ c) + beta @ (G @ beta)


def measure():
    """Prints what MEASURED_TIGHT and MEASURED_HELDOUT record."""
    worst_t = worst_h = 0.0
    for K in SWEEP_K:
        A, b, w, fold, _ = sweep_case(K)
        blocks = blocks_numpy(A, b, w, fold, SWEEP_F)
        alphas = alpha_grid(blocks, K, GRID4)
        coef, info, held = lp.lasso_path_host(blocks, K, alphas, MAX_ITER, TIGHT_TOL)
        folds, total = lp.sum_blocks(blocks)
        kt = kh = 0.0
        for f in range(SWEEP_F + 1):
            Qm, qv, y2, n, _ = lp.downdated(folds, total, f, K)
            for q, alpha in enumerate(alphas):
                wn, _, _ = cd_numpy(Qm, qv, y2, alpha * n, MAX_ITER, TIGHT_TOL)
                nrm = np.linalg.norm(coef[f, q])
                if nrm > 0:
                    kt = max(kt, np.linalg.norm(wn - coef[f, q]) / nrm)
                if f < SWEEP_F:
                    ref = heldout_ld(A, b, w, np.flatnonzero(fold == f), coef[f, q])
                    kh = max(kh, abs(heldout_numpy(folds[f], K, coef[f, q]) - ref) / ref)
        print(f"K = {K:3d}  restatement vs oracle A {kt:.2e}   three-term vs long double {kh:.2e}  max sweeps {int(info[:, :, 0].max())}",
              flush=True)
        worst_t, worst_h = max(worst_t, kt), max(worst_h, kh)
    print(f"MEASURED_TIGHT = {worst_t:.1e}  MEASURED_HELDOUT = {worst_h:.1e}")


if __name__ == "__main__":
    measure()
