"""Cases, generators, the long-double reference and the bars of the robust (IRLS) tests -- tests/test_robust_cpu.py and
tests/test_gpu_robust.py.

The reference restates the whole iteration of fitsnap_amd/solvers/robust.py in ``np.longdouble`` with an explicit weighted
Gram matrix and an explicit Cholesky factorisation (numpy's LAPACK calls are fp64 only): residuals, per-class medians,
r = sqrt(omega) by the closed forms, the ridge fit.  Nothing here imports the code under test."""
from __future__ import annotations

import functools

import numpy as np

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
MAD_TO_SIGMA = LD("1.4826")
DEFAULT_TUNE = {"huber": 1.345, "bisquare": 4.685, "cauchy": 2.385}
LOSSES = ("huber", "bisquare", "cauchy")

# class g: noise sigma_g of the truths, base weight w_g (the weighted noise 0.1 / 0.05 / 0.02 still differs per class)
CLASS_NOISE = (1e-3, 5e-2, 2.0)
CLASS_WEIGHT = (100.0, 1.0, 1e-2)
CLASS_SHARE = (0.15, 0.55, 0.30)

# the end-to-end shapes (m, K) and the fixed iteration count of the accuracy comparisons
SHAPES = ((3000, 17), (5000, 33), (4000, 128))
FIXED_ITERS = 12
ALPHA = 1e-8

# max |robust_host - long double| / max |long double| after FIXED_ITERS iterations (tol = 0), measured with
# tests/test_robust_cpu.py::test_host_matches_long_double (which prints it); the prototype of the algorithm gave <= 5e-13.
# test_robust_cpu asserts <= HOST_BAR; the GPU's end-to-end bar is max(GPU_FLOOR, 100 x the entry).
HOST_BAR = 1e-11
GPU_FLOOR = 1e-10
HOST_DISTANCE = {
    (3000, 17, "huber"): 1.7e-15, (3000, 17, "bisquare"): 6.1e-16, (3000, 17, "cauchy"): 1.7e-15,
    (5000, 33, "huber"): 1.3e-15, (5000, 33, "bisquare"): 1.5e-15, (5000, 33, "cauchy"): 1.4e-15,
    (4000, 128, "huber"): 1.2e-15, (4000, 128, "bisquare"): 2.3e-15, (4000, 128, "cauchy"): 1.9e-15,
}


def gpu_bar(m, K, loss):
    return max(GPU_FLOOR, 100.0 * HOST_DISTANCE[(m, K, loss)])


class Case:
    """Rows with three classes whose noise differs by three decades, column scales 10^+-1, 5 % gross outliers of 20 - 200
    sigma, 10 % test rows and 2 % zero weights."""

    def __init__(self, m, K, seed=None):
        rng = np.random.default_rng(1000 * K + m if seed is None else seed)
        self.m, self.K = m, K
        colscale = 10.0 ** rng.uniform(-1.0, 1.0, K)
        self.A = rng.standard_normal((m, K)) * colscale
        self.truth = rng.standard_normal(K) / colscale
        self.cat = rng.choice(3, size=m, p=CLASS_SHARE).astype(np.int32)
        sigma = np.asarray(CLASS_NOISE)[self.cat]
        self.b = self.A @ self.truth + sigma * rng.standard_normal(m)
        self.outliers = np.sort(rng.choice(m, size=max(1, m // 20), replace=False))
        self.b[self.outliers] += rng.choice([-1.0, 1.0], size=len(self.outliers)) * rng.uniform(20.0, 200.0, len(self.outliers)) \
            * sigma[self.outliers]
        self.mask = rng.random(m) >= 0.1
        self.w = np.asarray(CLASS_WEIGHT)[self.cat].copy()
        self.w[rng.choice(m, size=max(1, m // 50), replace=False)] = 0.0
        self.part = self.mask & (self.w > 0.0)
        self.row_type = np.array(["Energy", "Force", "Stress"])[self.cat]

    def fs_dict(self):
        """Labels as a calculator leaves them: 13 rows per configuration, four groups."""
        cfg = np.arange(self.m) // 13
        return {"Testing": (~self.mask).tolist(), "Row_Type": self.row_type.tolist(), "Configs": [f"cfg{c}" for c in cfg],
                "Groups": [f"grp{c % 4}" for c in cfg]}


@functools.lru_cache(maxsize=None)
def case(m, K):
    return Case(m, K)


def probe_beta(cs):
    """A coefficient vector near the truth (1 % off per entry): what the kernel tests evaluate residuals at."""
    return cs.truth * (1.0 + 0.01 * np.random.default_rng(7).standard_normal(cs.K))


# ---- the closed forms, in long double ---------------------------------------------------------------------------------

def ref_weight(loss, c, s, e):
    """(r, rho) per row in long double from residuals e and per-row scales s; s == 0: r = 1, rho = 0."""
    e = np.asarray(e, dtype=LD)
    s = np.broadcast_to(np.asarray(s, dtype=LD), e.shape)
    c = LD(c)
    r = np.ones(e.shape, dtype=LD)
    rho = np.zeros(e.shape, dtype=LD)
    for i in np.flatnonzero(s > 0):
        cs, ae, u = c * s[i], abs(e[i]), e[i] / s[i]
        if loss == "huber":
            if ae <= cs:
                rho[i] = u * u / 2
            else:
                r[i] = np.sqrt(cs / ae)
                rho[i] = c * abs(u) - c * c / 2
        elif loss == "bisquare":
            if ae < cs:
                r[i] = 1 - (e[i] / cs) ** 2
                rho[i] = c * c / 6 * (1 - (1 - (u / c) ** 2) ** 3)
            else:
                r[i] = 0
                rho[i] = c * c / 6
        elif loss == "cauchy":
            r[i] = 1 / np.sqrt(1 + (e[i] / cs) ** 2)
            rho[i] = c * c / 2 * np.log(1 + (u / c) ** 2)
        else:
            raise ValueError(loss)
    return r, rho


def ref_weight_vec(loss, c, s, e):
    """``ref_weight`` vectorised (the iteration below calls it on thousands of rows)."""
    e = np.asarray(e, dtype=LD)
    s = np.broadcast_to(np.asarray(s, dtype=LD), e.shape)
    c = LD(c)
    ok = s > 0
    so = np.where(ok, s, LD(1))
    cs, ae, u = c * so, np.abs(e), e / so
    if loss == "huber":
        inside = ae <= cs
        r = np.where(inside, LD(1), np.sqrt(cs / np.where(inside, LD(1), ae)))
        rho = np.where(inside, u * u / 2, c * np.abs(u) - c * c / 2)
    elif loss == "bisquare":
        inside = ae < cs
        r = np.where(inside, 1 - (e / cs) ** 2, LD(0))
        rho = np.where(inside, c * c / 6 * (1 - (1 - (u / c) ** 2) ** 3), c * c / 6)
    elif loss == "cauchy":
        r = 1 / np.sqrt(1 + (e / cs) ** 2)
        rho = c * c / 2 * np.log(1 + (u / c) ** 2)
    else:
        raise ValueError(loss)
    return np.where(ok, r, LD(1)), np.where(ok, rho, LD(0))


def ref_scales(e, cat, ncat):
    """1.4826 x median |e| per class in long double (numpy's median: the mean of the two middle values); 0 when empty."""
    s = np.zeros(ncat, dtype=LD)
    ae = np.abs(np.asarray(e, dtype=LD))
    for g in range(ncat):
        sel = cat == g
        if sel.any():
            s[g] = MAD_TO_SIGMA * np.median(ae[sel])
    return s


def ref_table(e, r, rho, cat, ncat):
    out = np.zeros((ncat, 6), dtype=LD)
    for g in range(ncat):
        sel = cat == g
        out[g] = (np.count_nonzero(sel), np.count_nonzero(r[sel] < 1), np.count_nonzero(r[sel] == 0), np.sum(r[sel] * r[sel]),
                  np.sum(e[sel] * e[sel]), np.sum(rho[sel]))
    return out


EXPLICIT_MAX_K = 64


def ld_ridge(X, y, alpha):
    """argmin |X beta - y|^2 + alpha |beta|^2 to long-double accuracy.  Up to EXPLICIT_MAX_K columns by ``ld_ridge_explicit``;
    wider systems by ``ld_ridge_refined``, which reaches the same minimiser without the long-double Gram matrix (numpy forms
    it without BLAS: 0.8 s per fit at 4000 x 128, 13 fits per run).  test_robust_cpu checks that the two agree."""
    return ld_ridge_explicit(X, y, alpha) if X.shape[1] <= EXPLICIT_MAX_K else ld_ridge_refined(X, y, alpha)


def ld_ridge_refined(X, y, alpha, steps=8):
    """The minimiser as the fixed point of x += (G64 + alpha I)^-1 (X^T (y - X x) - alpha x): the gradient in long double
    from the rows (two matrix-vector products), the correction through an fp64 Cholesky factor of the fp64 Gram matrix.
    Every step contracts the error by ~kappa(G) eps64; the loop ends when a step no longer changes x in long double."""
    X64 = np.asarray(X, dtype=np.float64)
    K = X.shape[1]
    G = X64.T @ X64
    G[np.diag_indices(K)] += float(alpha)
    d = np.sqrt(np.diag(G))
    Lc = np.linalg.cholesky(G / d[:, None] / d[None, :])
    x = np.zeros(K, dtype=LD)
    for _ in range(steps):
        g = X.T @ (y - X @ x) - LD(alpha) * x
        z = np.linalg.solve(Lc.T, np.linalg.solve(Lc, np.asarray(g / d, dtype=np.float64))) / d
        x = x + np.asarray(z, dtype=LD)
        if np.max(np.abs(z)) <= 1e-20 * float(np.max(np.abs(x))):
            break
    return x


def ld_ridge_explicit(X, y, alpha):
    """The same in long double throughout: explicit Gram matrix, Jacobi scaling, explicit Cholesky."""
    K = X.shape[1]
    G = X.T @ X
    G[np.diag_indices(K)] += LD(alpha)
    c = X.T @ y
    d = np.sqrt(np.diag(G))
    S = G / d[:, None] / d[None, :]
    L = np.zeros((K, K), dtype=LD)
    for j in range(K):
        L[j, j] = np.sqrt(S[j, j] - L[j, :j] @ L[j, :j])
        if j + 1 < K:
            L[j + 1:, j] = (S[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    z = np.zeros(K, dtype=LD)
    rhs = c / d
    for j in range(K):
        z[j] = (rhs[j] - L[j, :j] @ z[:j]) / L[j, j]
    x = np.zeros(K, dtype=LD)
    for j in range(K - 1, -1, -1):
        x[j] = (z[j] - L[j + 1:, j] @ x[j + 1:]) / L[j, j]
    return x / d


def reference(A, b, w, mask, cat, ncat, loss, tune=None, alpha=ALPHA, max_iter=FIXED_ITERS, tol=0.0, scale=None, scale_iters=0,
              start=None):
    """The whole iteration in long double.  Returns dict(fit, iterations, converged, scales, tables, omega, start)."""
    c = DEFAULT_TUNE[loss] if tune is None else tune
    mask = np.ones(len(b), dtype=bool) if mask is None else np.asarray(mask, dtype=bool)
    cat = np.zeros(len(b), dtype=np.int64) if cat is None else np.asarray(cat)
    part = mask & (np.asarray(w) > 0)
    Ap, bp, wp, cp = np.asarray(A, dtype=LD)[part], np.asarray(b, dtype=LD)[part], np.asarray(w, dtype=LD)[part], cat[part]
    beta = ld_ridge(Ap * wp[:, None], bp * wp, alpha) if start is None else np.asarray(start, dtype=LD)
    beta0 = beta.copy()
    s = np.zeros(ncat, dtype=LD) if scale is None else np.asarray(scale, dtype=LD)
    scales, tables, it, converged = [], [], 0, False
    r = np.ones(len(bp), dtype=LD)
    for t in range(max_iter):
        e = wp * (bp - Ap @ beta)
        if scale is None and (scale_iters == 0 or t < scale_iters):
            s = ref_scales(e, cp, ncat)
        r, rho = ref_weight_vec(loss, c, s[cp], e)
        scales.append(s.copy())
        tables.append(ref_table(e, r, rho, cp, ncat))
        wr = wp * r
        new = ld_ridge(Ap * wr[:, None], bp * wr, alpha)
        it = t + 1
        done = np.max(np.abs(new - beta)) <= LD(tol) * np.max(np.abs(new))
        beta = new
        if done:
            converged = True
            break
    omega = np.ones(len(b), dtype=LD)
    omega[part] = r * r
    return {"fit": beta, "iterations": it, "converged": converged, "scales": np.array(scales), "tables": np.array(tables),
            "omega": omega, "start": beta0}


@functools.lru_cache(maxsize=None)
def reference_of(m, K, loss):
    """The long-double run of the standard case (m, K) with ``loss``: FIXED_ITERS iterations, tol = 0.  Computed once."""
    cs = case(m, K)
    return reference(cs.A, cs.b, cs.w, cs.mask, cs.cat, 3, loss)


def distance(beta, ref):
    ref = np.asarray(ref, dtype=LD)
    return float(np.max(np.abs(np.asarray(beta, dtype=LD) - ref)) / np.max(np.abs(ref)))


# ---- bars of the kernel tests --------------------------------------------------------------------------------------------

def residual_bar(A, b, w, beta):
    """A priori bound per row of |e_i - e_i(long double)| for e_i = w_i (b_i - a_i . beta): 4 eps (K + 2) w_i (|a_i| . |beta| + |b_i|)."""
    K = A.shape[1]
    return 4.0 * EPS * (K + 2) * np.abs(w) * (np.abs(A) @ np.abs(beta) + np.abs(b))


def residual_reference(A, b, w, part, beta):
    e = np.asarray(w, dtype=LD) * (np.asarray(b, dtype=LD) - np.asarray(A, dtype=LD) @ np.asarray(beta, dtype=LD))
    return np.where(part, e, LD(0))
