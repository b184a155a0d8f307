"""Pools for the batch-selection tests (tests/test_select_cpu.py, tests/test_gpu_select.py, tests/select_dist_worker.py) and
their reference: per-step REFITS, independent of the downdate algebra of fitsnap_amd/solvers/select.py.

Pools cluster, so that redundancy exists: every configuration sits at one of six random centres (rows = 0.7 centre + unit
Gaussian noise, column scales 0.5 ... 2, weights 0.5 ... 2, 1 ... 300 rows per configuration); the prior comes from a training
set of 40 ... 60 such configurations: information matrix P0 = Aw^T Aw + nugget I, covariance C0 = tau pinv(P0).

Reference after the units u_1 ... u_t:  C_t = tau pinv(P0 + sum X_u^T X_u) (float64; P0 = tau C0^-1 by construction, over
the non-zero columns), variances diag(A C_t A^T), aggregation by bincount / maximum.at, arg-max with ties to the first key.
"""
import numpy as np

EPS = np.finfo(np.float64).eps


def clustered(seed, K, n_train=50, n_pool=200, size_lo=1, size_hi=300, zero_col=None, nugget=1e-8, tau=0.04):
    """dict: pool rows "A", weights "w", categories "cat" (int32, one id per configuration), "ncat", scale "s", the prior
    "P0" / "C0" / "tau", and the training rows "At", "wt"."""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((6, K))
    colscale = rng.uniform(0.5, 2.0, K)
    if zero_col is not None:
        colscale[zero_col] = 0.0

    def block(ncfg):
        sizes = rng.integers(size_lo, size_hi + 1, ncfg)
        which = rng.integers(0, 6, ncfg)
        m = int(sizes.sum())
        rows = (0.7 * np.repeat(centres[which], sizes, axis=0) + rng.standard_normal((m, K))) * colscale
        return rows, rng.uniform(0.5, 2.0, m), np.repeat(np.arange(ncfg), sizes).astype(np.int32)

    At, wt, _ = block(n_train)
    A, w, cat = block(n_pool)
    Aw = At * wt[:, None]
    P0 = Aw.T @ Aw + nugget * np.eye(K)
    if zero_col is not None:
        P0[zero_col, :] = 0.0
        P0[:, zero_col] = 0.0
    C0 = tau * np.linalg.pinv(P0, hermitian=True)
    C0 = 0.5 * (C0 + C0.T)
    return {"A": np.ascontiguousarray(A), "w": w, "cat": cat, "ncat": int(n_pool), "s": rng.uniform(0.5, 2.0, A.shape[0]),
            "P0": P0, "C0": C0, "tau": tau, "At": At, "wt": wt}


def info_inverse(P):
    """(pinv of the information matrix over its non-zero columns, its condition number there)."""
    nz = np.flatnonzero(np.diag(P) != 0.0)
    blk = P[np.ix_(nz, nz)]
    out = np.zeros_like(P)
    out[np.ix_(nz, nz)] = np.linalg.pinv(blk, hermitian=True)
    return out, float(np.linalg.cond(blk))


def aggregate(val, cat, ncat, objective):
    use = cat >= 0
    c = cat[use].astype(np.int64)
    count = np.bincount(c, minlength=ncat)
    if objective == "max":
        out = np.full(ncat, -np.inf)
        np.maximum.at(out, c, val[use])
        return out, count
    s = np.bincount(c, weights=val[use], minlength=ncat)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (s / count if objective == "mean" else s), count


def refit_reference(A, cat, ncat, P0, tau, w, batch_size, scale=None, objective="sum"):
    """Greedy selection by refits.  dict: "picks", "scores", "gaps" (relative gap between the best and the second-best live
    score at every step; inf with one live category), "kappa" (condition number of the matrix inverted for the state BEFORE
    step t, t = 0 ... picks), "var" (variances before step t, t = 0 ... picks), "cov" (likewise), "initial" (scores before
    the first pick)."""
    A = np.asarray(A, dtype=np.float64)
    cat = np.asarray(cat)
    scale = np.ones(A.shape[0]) if scale is None else np.asarray(scale, dtype=np.float64)
    P = np.array(P0, dtype=np.float64)
    count = np.bincount(cat[cat >= 0].astype(np.int64), minlength=ncat)
    alive = count > 0
    res = {"picks": [], "scores": [], "gaps": [], "kappa": [], "var": [], "cov": [], "initial": None}
    for t in range(int(batch_size) + 1):
        Pinv, kappa = info_inverse(P)
        C = tau * Pinv
        var = np.einsum("ij,ij->i", A @ C, A)
        res["kappa"].append(kappa)
        res["var"].append(var)
        res["cov"].append(C)
        sc, _ = aggregate(scale * var, cat, ncat, objective)
        if t == 0:
            res["initial"] = sc.copy()
        if t == int(batch_size) or not alive.any():
            break
        live = np.flatnonzero(alive)
        order = live[np.argsort(-sc[live], kind="stable")]           # ties: the first key
        u = int(order[0])
        gap = np.inf if len(order) < 2 else float((sc[order[0]] - sc[order[1]]) / abs(sc[order[0]]))
        res["picks"].append(u)
        res["scores"].append(float(sc[u]))
        res["gaps"].append(gap)
        alive[u] = False
        X = w[cat == u, None] * A[cat == u]
        P = P + X.T @ X
    return res


def kernel_bar(A, C0, factors):
    """Rounding bar of the resident variances after begin (QUAD with C0) and the downdates with ``factors``, per row, in the
    form of ref_long of tests/test_gpu_uq.py, accumulated: 4 eps [K (|a| |C0| |a|) + sum_t (K + J_t) || |a| |V_t| ||^2]."""
    aa = np.abs(np.asarray(A, dtype=np.float64))
    K = aa.shape[1]
    bar = 4 * K * EPS * ((aa @ np.abs(C0)) * aa).sum(axis=1)
    for V in factors:
        bar = bar + 4 * (K + V.shape[1]) * EPS * ((aa @ np.abs(V)) ** 2).sum(axis=1)
    return bar


def long_double_var(A, C0, factors):
    """a^T C0 a - sum_t ||a V_t||^2 in long double."""
    al = np.asarray(A).astype(np.longdouble)
    v = ((al @ np.asarray(C0).astype(np.longdouble)) * al).sum(axis=1)
    for V in factors:
        T = al @ np.asarray(V).astype(np.longdouble)
        v = v - (T * T).sum(axis=1)
    return v.astype(np.float64)


def ta_configurations(m, seed=5, lo=1, hi=120):
    """Synthetic configuration ids for the first m golden Ta rows: consecutive blocks of lo ... hi rows."""
    rng = np.random.default_rng(seed)
    sizes = []
    while sum(sizes) < m:
        sizes.append(int(rng.integers(lo, hi + 1)))
    sizes[-1] -= sum(sizes) - m
    return np.repeat(np.arange(len(sizes)), sizes).astype(np.int32), len(sizes)
