"""Host side of greedy active-learning batch selection (``Solver.select_batch``; ``fsnap_select_*``, csrc/fsnap_select.hip).

With a linear model and a Gaussian posterior the predictive variance of a row, ``a^T C a``, does not depend on the labels,
so the posterior AFTER a unit (normally one configuration) has been added to the training set is known before its labels
exist.  With X = diag(omega_u) A_u (d x K) the weighted rows of the picked unit u and unit-weight noise tau:

    Z = C X^T,   S = tau I_d + X Z = L L^T,   V = Z L^-T  (K x d),   C' = C - V V^T
    var_i' = var_i - ||a_i V||^2                                     (the pass over the pool rows, kernel B1)

For ANL, C = sigma^2 pinv(G + nugget I) and tau = sigma^2 give exactly C' = sigma^2 (G + nugget I + X^T X)^-1.  S is positive
definite for any PSD C, so a pinv covariance with zero columns needs no special case.  When d > K the GPU gets J = K columns:
V V^T depends on X through X^T X alone, so the K x K triangle R of a QR factorisation of X replaces X before anything else
is formed (the same V V^T as R^T of a QR of V^T, without the d x d Cholesky).  J = min(d, K) in every case.

Pure numpy, so that it can be checked without a GPU: ``greedy_host`` is the whole loop with ``fold`` (the kernel's formula)
in place of the GPU pass; ``select_batch`` is the same loop on the resident rows, collective over several ranks.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from .._hostblas import blas_threads
from . import uq

OBJECTIVES = ("sum", "max", "mean")          # the reference's objective_function options sum / max / average

BatchSelection = namedtuple("BatchSelection", "keys scores all_keys initial_scores var cov ranks")
BatchSelection.__doc__ = """Result of ``Solver.select_batch``: ``keys`` the picked categories in order, ``scores`` each pick's
score at the moment it was picked, ``all_keys`` / ``initial_scores`` the one-shot ranking of every category (this rank's),
``var`` this rank's per-row variances after the last pick, ``cov`` the posterior covariance after the last pick, ``ranks``
the number of columns J of every pick's factor."""


def check_objective(objective):
    """The objective's name ("average" is the reference's word for "mean"); ValueError for anything else."""
    name = "mean" if objective == "average" else objective
    if name not in OBJECTIVES:
        raise ValueError(f"objective must be one of {OBJECTIVES} (or 'average'), not {objective!r}")
    return name


def check_noise(noise):
    noise = float(noise)
    if not noise > 0.0 or not np.isfinite(noise):
        raise ValueError(f"noise must be a positive variance, not {noise}")
    return noise


def category_layout(categories):
    """(int32 ids per row, keys) from int ids (negative = the row takes no part; keys = range(ncat)), one label per row, or
    a tuple of per-row label columns -- the forms of ``Solver.prediction_variance``."""
    if categories is None:
        raise ValueError("select_batch needs categories: the units to pick from")
    arr = None if isinstance(categories, tuple) else np.asarray(categories)
    if arr is not None and arr.ndim == 1 and np.issubdtype(arr.dtype, np.integer):
        cat = arr.astype(np.int32)
        ncat = int(cat.max()) + 1 if cat.size and cat.max() >= 0 else 0
        return cat, list(range(ncat))
    return uq.category_ids(categories)


def downdate_factor(cov, X, noise):
    """V (K x J, J = min(d, K)) with cov - V V^T the posterior given the d rows X with unit-weight noise ``noise``.  The rows
    enter the posterior through X^T X alone, so for d > K the K x K triangle R of a QR factorisation of X (R^T R = X^T X)
    stands in for X: the same V V^T as R^T of a QR of the d-column factor's transpose, with K x K algebra only."""
    from scipy.linalg import solve_triangular

    C = np.asarray(cov, dtype=np.float64)
    X = np.asarray(X, dtype=np.float64).reshape(-1, C.shape[0])
    K = C.shape[0]
    with blas_threads(K):
        if X.shape[0] > K:
            X = np.linalg.qr(X, mode="r")
        Z = C @ X.T
        S = X @ Z
        S = 0.5 * (S + S.T)
        S[np.diag_indices_from(S)] += noise
        L = np.linalg.cholesky(S)
        Vt = solve_triangular(L, Z.T, lower=True, check_finite=False)      # V^T = L^-1 Z^T   (J x K)
    return np.ascontiguousarray(Vt.T)


def downdate_cov(cov, V):
    """cov - V V^T, symmetric."""
    C = np.asarray(cov, dtype=np.float64) - V @ V.T
    return 0.5 * (C + C.T)


def fold(a, V):
    """What kernel B1 subtracts from a row's variance, in numpy: ((a V)^2).sum(1)."""
    T = np.asarray(a, dtype=np.float64) @ V
    return (T * T).sum(axis=1)


def aggregate(var, scale, cat, ncat):
    """Per-category (sum, max, count) of scale_i var_i over the rows with cat >= 0 (an empty category: 0, -inf, 0)."""
    cat = np.asarray(cat)
    use = cat >= 0
    val = np.asarray(var, dtype=np.float64)[use]
    if scale is not None:
        val = np.asarray(scale, dtype=np.float64)[use] * val
    c = cat[use].astype(np.int64)
    sums = np.bincount(c, weights=val, minlength=ncat).astype(np.float64)
    maxs = np.full(ncat, -np.inf)
    np.maximum.at(maxs, c, val)
    return sums, maxs, np.bincount(c, minlength=ncat).astype(np.int64)


def scores_of(cat_sum, cat_max, cat_count, objective):
    """Score per category from its (sum, max, count): the sum, the max or sum / count."""
    if objective == "sum":
        return np.array(cat_sum, dtype=np.float64)
    if objective == "max":
        return np.array(cat_max, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.asarray(cat_sum, dtype=np.float64) / np.asarray(cat_count)


def best_live(scores, alive):
    """Index of the largest score among the live categories, ties to the first in key order, a NaN score ranking lowest;
    -1 when none is alive."""
    alive = np.asarray(alive, dtype=bool)
    if not alive.any():
        return -1
    key = np.where(np.isnan(scores), -np.inf, scores)
    key = np.where(alive, key, -np.inf)
    top = key.max()
    return int(np.flatnonzero(alive & (key == top))[0])


def best_of_ranks(pairs):
    """(rank, category) of the winner among the ranks' local picks ``pairs`` = [(score, category or -1), ...]: the largest
    score, ties to the lowest rank -- the first key in rank-major key order; (-1, -1) when no rank has a live category."""
    best = (-1, -1)
    top = None
    for r, (s, c) in enumerate(pairs):
        if c < 0:
            continue
        k = -np.inf if s != s else s
        if top is None or k > top:
            best, top = (r, c), k
    return best


def greedy_host(a, cat, ncat, cov, w, noise, batch_size, scale=None, objective="sum"):
    """The whole selection in numpy (float64): what ``select_batch`` computes with the GPU passes replaced by ``fold`` and
    ``aggregate``.  Returns a dict: "picks" (category ids), "scores", "gaps" (relative gap to the second-best live score at
    every pick; inf with one live category), "ranks", "factors" (the V of every pick), "var", "cov", "initial" ((sum, max,
    count) before the first pick) and "alive"."""
    objective = check_objective(objective)
    noise = check_noise(noise)
    if int(batch_size) < 0:
        raise ValueError("batch_size must not be negative")
    a = np.asarray(a, dtype=np.float64)
    C = np.array(cov, dtype=np.float64)
    cat = np.asarray(cat)
    w = np.ones(a.shape[0]) if w is None else np.asarray(w, dtype=np.float64).reshape(-1)
    var = uq.fold(a, uq.QUAD, C)
    sums, maxs, count = aggregate(var, scale, cat, ncat)
    initial = (sums.copy(), maxs.copy(), count.copy())
    alive = count > 0
    picks, scores, gaps, ranks, factors = [], [], [], [], []
    for _ in range(int(batch_size)):
        sc = scores_of(sums, maxs, count, objective)
        u = best_live(sc, alive)
        if u < 0:
            break
        alive[u] = False
        rest = sc[alive]
        gaps.append(float((sc[u] - rest.max()) / abs(sc[u])) if rest.size else np.inf)
        rows = np.flatnonzero(cat == u)
        V = downdate_factor(C, w[rows, None] * a[rows], noise)
        C = downdate_cov(C, V)
        var = var - fold(a, V)
        s2, m2, _ = aggregate(var, scale, cat, ncat)
        sums = np.where(alive, s2, sums)         # retired categories keep the values they were retired with
        maxs = np.where(alive, m2, maxs)
        picks.append(u)
        scores.append(float(sc[u]))
        ranks.append(V.shape[1])
        factors.append(V)
    return {"picks": picks, "scores": scores, "gaps": gaps, "ranks": ranks, "factors": factors, "var": var, "cov": C, "initial": initial,
            "alive": alive}


def select_batch(solver, batch_size, a=None, w=None, categories=None, row_scale=None, objective="sum", noise=None, cov=None,
                 keep_factors=False):
    """``Solver.select_batch``: see there.  ``keep_factors`` leaves the V of every pick in ``solver._select_factors``."""
    from .. import _capi

    pt = solver.pt
    objective = check_objective(objective)
    if int(batch_size) < 0:
        raise ValueError("batch_size must not be negative")
    C = cov if cov is not None else solver.cov
    noise = noise if noise is not None else getattr(solver, "sigmahat", None)
    if pt.multi:
        C, noise = pt.bcast_object((C, noise), src=0)         # rank 0's, where the fit lives
    if C is None:
        raise ValueError("select_batch: no posterior covariance (fit ANL first, or pass cov=)")
    if noise is None:
        raise ValueError("select_batch: no noise variance (the sigma^2 of an ANL fit is kept; otherwise pass noise=)")
    noise = check_noise(noise)
    C = np.array(C, dtype=np.float64)
    if C.ndim != 2 or C.shape[0] != C.shape[1]:
        raise ValueError("cov must be K x K")
    cat, keys = category_layout(categories)
    ncat = len(keys)
    rows_host = pt.shared_arrays["a"].array if a is None else np.asarray(a)
    m = rows_host.shape[0]
    if cat.shape[0] != m:
        raise ValueError(f"{cat.shape[0]} categories for {m} rows")
    if m > 0 and rows_host.shape[1] != C.shape[0]:
        raise ValueError(f"cov is {C.shape[0]} x {C.shape[0]}, the rows have {rows_host.shape[1]} columns")
    if w is None:
        w = pt.shared_arrays["w"].array if a is None else np.ones(m)
    w = np.asarray(w, dtype=np.float64).reshape(-1)
    if w.shape[0] != m:
        raise ValueError(f"{w.shape[0]} weights for {m} rows")
    if pt.multi:
        from . import loco
        try:
            loco.check_units_disjoint(pt.allgather_object(list(keys)))
        except ValueError as e:
            raise ValueError(str(e).replace("loco_errors", "select_batch")) from None
    session = ncat > 0
    ctx = solver._uq_rows(a) if session else None
    if session:
        ctx.select_begin(C, _capi.UQ_QUAD, scale=row_scale, cat=cat, ncat=ncat, objective=_capi.SELECT_OBJECTIVES[objective])
        st = ctx.select_state(want_var=False)
        initial = scores_of(st["cat_sum"], st["cat_max"], st["cat_count"], objective)
        order = np.argsort(cat, kind="stable")
        first = np.searchsorted(cat[order], np.arange(ncat + 1))
    else:
        initial = np.zeros(0)
    picked, scores, ranks, factors = [], [], [], []
    try:
        for _ in range(int(batch_size)):
            if pt.multi:
                c, s = ctx.select_pick(retire=False) if session else (-1, 0.0)
                pairs = pt.allgather_object((s, c))
                owner, c = best_of_ranks(pairs)
                if owner < 0:
                    break
                s = pairs[owner][0]
                msg = None
                if owner == pt._rank:
                    ctx.select_retire(c)
                    rows = order[first[c]:first[c + 1]]
                    msg = (keys[c], w[rows, None] * np.asarray(rows_host[rows], dtype=np.float64))
                key, X = pt.bcast_object(msg, src=owner)
            else:
                if not session:
                    break
                c, s = ctx.select_pick(retire=True)
                if c < 0:
                    break
                rows = order[first[c]:first[c + 1]]
                key, X = keys[c], w[rows, None] * np.asarray(rows_host[rows], dtype=np.float64)
            V = downdate_factor(C, X, noise)
            C = downdate_cov(C, V)
            if session:
                ctx.select_downdate(V)
            picked.append(key)
            scores.append(float(s))
            ranks.append(V.shape[1])
            if keep_factors:
                factors.append(V)
        var = ctx.select_state()["var"] if session else np.zeros(m)
    finally:
        if session:
            ctx.select_end()
    if keep_factors:
        solver._select_factors = factors
    return BatchSelection(picked, np.array(scores), list(keys), initial, var, C, ranks)
