"""Cases and references for the joint unit scores (tests/test_select_joint_cpu.py, tests/test_gpu_select_joint.py,
tests/select_joint_dist_worker.py): fitsnap_amd/solvers/select_joint.py and the kernels of csrc/fsnap_joint.hip.

Two references, neither of which shares algebra with the code under test:

* BY REFITS (``refit_scores``, ``refit_greedy``), from the information matrix P (C = tau pinv(P)):
      reduction_u = tr(T (C - C'_u)),  C'_u = tau pinv(P + X^T X)                        (float64)
      gain_u      = 1/2 sum log(1 + lambda) over the generalised eigenvalues of (X^T X, P), the log1p in long double
  (a plain slogdet difference cancels: it is 10^3 kappa eps off on its own and is not used).  Its own error is that of the
  inverse of a matrix of condition kappa: kappa eps relative in C and C', hence kappa eps tr(T C) absolute in the reduction,
  and kappa eps lambda_max in every eigenvalue, hence at most kappa eps (rows of the unit) in the gain.  ``REFIT_C`` = 16 is
  the constant that tests/test_gpu_select.py puts in front of kappa eps for the same kind of reference.

* IN LONG DOUBLE (``long_double_scores``): the kernel's own formulas, given the same M, B and tau, with every product,
  the Cholesky factor and the substitution in numpy long double (64-bit mantissa).  ``rounding_bound`` is the bound of a
  float64 evaluation derived from the term counts, in the manner of ``select_cases.kernel_bar``: 4 eps x (number of terms
  of the longest sum chain) x (the same expression with absolute values in place of every factor).
"""
import numpy as np

import select_cases as sc

EPS = sc.EPS
REFIT_C = 16
LD = np.longdouble

# (seed, K, units, size_hi): the pools of the issue's probe; 8 greedy picks, target = pool Gram with the pool's s
POOLS = [(1, 31, 60, 120), (2, 64, 40, 200), (3, 128, 30, 300)]
PICKS = 8


def pool(seed, K, units, size_hi, **kw):
    p = sc.clustered(seed, K, n_pool=units, size_hi=size_hi, **kw)
    p["T"] = p["A"].T @ (p["s"][:, None] * p["A"])
    return p


# ---------------------------------------------------------------------------------------------------------------------
# reference by refits
# ---------------------------------------------------------------------------------------------------------------------
def refit_scores(A, cat, ncat, P, tau, w, T, alive=None):
    """(gain, reduction, kappa) of every live unit by refits from the information matrix P; kappa = cond(P) over its non-zero
    columns.  Empty units score 0, units that are not alive NaN."""
    from scipy.linalg import eigh

    nz = np.flatnonzero(np.diag(P) != 0.0)
    Pn = P[np.ix_(nz, nz)]
    Pinv, kappa = sc.info_inverse(P)
    C = tau * Pinv
    gain = np.full(ncat, np.nan)
    red = np.full(ncat, np.nan)
    for u in range(ncat):
        if alive is not None and not alive[u]:
            continue
        sel = cat == u
        if not sel.any():
            gain[u] = red[u] = 0.0
            continue
        X = w[sel, None] * A[sel]
        XtX = X.T @ X
        C1 = tau * sc.info_inverse(P + XtX)[0]
        red[u] = np.trace(T @ (C - C1))
        Xn = X[:, nz]
        lam = eigh(Xn.T @ Xn, Pn, eigvals_only=True)
        gain[u] = float(0.5 * np.log1p(np.maximum(lam, 0.0).astype(LD)).sum())
    return gain, red, kappa


def refit_bars(A, cat, ncat, C, tau, w, T, kappa):
    """Absolute bars of ``refit_scores``'s own error per unit: (gain, reduction)."""
    count = np.bincount(cat[cat >= 0].astype(np.int64), minlength=ncat)
    return REFIT_C * kappa * EPS * np.maximum(count, 1), np.full(ncat, REFIT_C * kappa * EPS * abs(np.trace(T @ C)))


def refit_greedy(A, cat, ncat, P0, tau, w, batch, criterion, T, unit_cost=None):
    """Greedy selection by refits: dict of "picks", "scores", "gaps" (relative gap best / runner-up), "kappa" and "all" (the
    score arrays of every step) and "cov" (the covariance after the last pick)."""
    P = np.array(P0, dtype=np.float64)
    cost = np.ones(ncat) if unit_cost is None else np.asarray(unit_cost, dtype=np.float64)
    count = np.bincount(cat[cat >= 0].astype(np.int64), minlength=ncat)
    alive = count > 0
    res = {"picks": [], "scores": [], "gaps": [], "kappa": [], "all": []}
    for _ in range(batch):
        if not alive.any():
            break
        g, r, kappa = refit_scores(A, cat, ncat, P, tau, w, T, alive)
        s = (g if criterion == "gain" else r) / cost
        live = np.flatnonzero(alive)
        order = live[np.argsort(-s[live], kind="stable")]
        u = int(order[0])
        res["gaps"].append(np.inf if len(order) < 2 else float((s[order[0]] - s[order[1]]) / abs(s[order[0]])))
        res["picks"].append(u)
        res["scores"].append(float(s[u]))
        res["kappa"].append(kappa)
        res["all"].append(s)
        alive[u] = False
        X = w[cat == u, None] * A[cat == u]
        P = P + X.T @ X
    Pinv, kappa = sc.info_inverse(P)
    res["cov"] = tau * Pinv
    res["kappa"].append(kappa)
    return res


# ---------------------------------------------------------------------------------------------------------------------
# the kernel's formulas in long double, and the rounding bound of a float64 evaluation
# ---------------------------------------------------------------------------------------------------------------------
def chol_ld(S):
    d = S.shape[0]
    L = np.zeros((d, d), dtype=LD)
    for k in range(d):
        L[k, k] = np.sqrt(S[k, k] - L[k, :k] @ L[k, :k])
        if k + 1 < d:
            L[k + 1:, k] = (S[k + 1:, k] - L[k + 1:, :k] @ L[k, :k]) / L[k, k]
    return L


def solve_ld(L, P):
    Y = np.zeros(P.shape, dtype=LD)
    for k in range(L.shape[0]):
        Y[k] = (P[k] - L[k, :k] @ Y[:k]) / L[k, k]
    return Y


def long_double_scores(X, M, tau, B=None):
    """(gain, reduction or None, bound of the gain, bound of the reduction) of one unit with weighted rows X under C = M M^T:
    the formulas of csrc/fsnap_joint.hip in long double, in the space the kernel uses (n <= J: n space), and the rounding
    bounds of their float64 evaluation."""
    Xl, Ml = np.asarray(X).astype(LD), np.asarray(M).astype(LD)
    n, K = Xl.shape
    J = Ml.shape[1]
    taul = LD(tau)
    Z = Xl @ Ml
    nspace = n <= J
    S = (Z @ Z.T if nspace else Z.T @ Z) / taul + np.eye(min(n, J), dtype=LD)
    d = S.shape[0]
    L = chol_ld(S)
    gain = float(np.log(np.diag(L)).sum())
    # bounds: the chains are K terms (Z), J or n terms (S), d terms (factor, substitution) long
    terms = K + (J if nspace else n) + d
    Lf = L.astype(np.float64)
    Linv = np.linalg.inv(Lf)
    aS = (np.abs(Lf) @ np.abs(Lf).T)                             # |E| <= gamma |L| |L|^T, d logdet = tr(S^-1 E)
    gbound = 4 * terms * EPS * (0.5 * float((np.abs(Linv.T @ Linv) * aS).sum()) + float(np.abs(np.log(np.diag(Lf))).sum()))
    red = rbound = None
    if B is not None:
        Bl = np.asarray(B).astype(LD)
        aB = np.abs(np.asarray(B, dtype=np.float64))
        if nspace:
            Y = solve_ld(L, Z @ Bl)
            red = float((Y * Y).sum() / taul)
            aP = np.abs(np.asarray(X, dtype=np.float64)) @ (np.abs(np.asarray(M, dtype=np.float64)) @ aB)
            rbound = 4 * (terms + J) * EPS * float(((np.abs(Linv) @ aP) ** 2).sum()) / tau
        else:
            Y = solve_ld(L, Bl)
            red = float((Bl * Bl).sum() - (Y * Y).sum())
            rbound = 4 * terms * EPS * float((aB ** 2).sum() + ((np.abs(Linv) @ aB) ** 2).sum())
    return gain, red, gbound, rbound


# sizes of the units of a kernel case: 1 ... 300 rows, around every tile edge, around J and around 128 (the LDS limit)
EDGE_SIZES = [1, 2, 15, 16, 17, 31, 32, 33, 48, 63, 64, 65, 100, 127, 128, 129, 141, 142, 143, 159, 160, 161, 200, 257, 300]
KERNEL_KS = [31, 64, 128, 142, 160]


def kernel_case(K, seed=0, lda_pad=3):
    """A pool for the kernel tests: dict with rows "A" (a strided view, lda = K + lda_pad), "cat" (unit id per row in a random
    row order, -1 for rows that take no part), "ncat", weights "w", "C0", "tau", the factor "M" (K x J), target "T" and its
    block "B" (J x r); one empty unit and one unit of weight zero among them."""
    from fitsnap_amd.solvers import select_joint as sj

    rng = np.random.default_rng(1000 * K + seed)
    prior = sc.clustered(500 + K + seed, K, n_pool=1)
    sizes = [n for n in EDGE_SIZES if n not in (K - 1, K, K + 1)] + [K - 1, K, K + 1]
    sizes = list(rng.permutation(sizes))
    sizes.insert(5, 0)                                           # an empty unit
    ncat = len(sizes)
    cat = np.repeat(np.arange(ncat), sizes)
    cat = np.concatenate([cat, np.full(37, -1)])                 # rows that take no part
    cat = cat[rng.permutation(cat.size)].astype(np.int32)
    m = cat.size
    centres = rng.standard_normal((ncat + 1, K))
    big = np.zeros((m, K + lda_pad))
    big[:, :K] = (0.7 * centres[cat] + rng.standard_normal((m, K))) * rng.uniform(0.5, 2.0, K)
    A = big[:, :K]
    w = rng.uniform(0.5, 2.0, m)
    w[cat == 7] = 0.0                                            # a unit of weight zero
    M = sj.factor_cov(prior["C0"])
    s = rng.uniform(0.5, 2.0, m)
    T = A.T @ (np.where(cat >= 0, s, 0.0)[:, None] * A)
    B = M.T @ sj.target_factor(T).T
    return {"A": A, "cat": cat, "ncat": ncat, "w": w, "s": s, "C0": prior["C0"], "tau": prior["tau"], "M": M, "T": T, "B": B,
            "sizes": np.array(sizes)}


def long_double_case(p):
    """(gain, reduction, gain bound, reduction bound) per unit of a kernel case; an empty unit: NaN."""
    out = np.full((4, p["ncat"]), np.nan)
    for u in range(p["ncat"]):
        sel = p["cat"] == u
        if sel.any():
            out[:, u] = long_double_scores(p["w"][sel, None] * p["A"][sel], p["M"], p["tau"], p["B"])
    return out
