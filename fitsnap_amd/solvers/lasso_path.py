"""Grouped K-fold LASSO alpha paths (what LassoCV with a GroupKFold is to Lasso).

Coordinate descent touches the weighted training rows x_i = w_i a_i, y_i = w_i b_i only through (X^T X, X^T y, |y|^2).  With
the units (configurations, or any label such as a group) dealt into F folds and one packed block [G_f | c_f | bb_f, sum wb,
n_f] per fold -- ONE pass over the rows, ``fsnap_cat_prepare`` + ``fsnap_cat_normal_eq`` with category = fold x row class --, the
training system of fold f is "total minus block f":

    Qm = T.G - G_f,  qv = T.c - c_f,  y2 = T.bb - bb_f,  n = T.n - n_f,  l1_reg = alpha_q n

which is scikit-learn's objective 1/(2n) |y - X w|^2 + alpha |w|_1 on the rows that remain (what ``LASSO.perform_fit`` hands
to ``fsnap_lasso_gram``).  Coordinate j is DEAD in a refit -- skipped, coefficient 0 -- when T.G_jj == 0 or Qm_jj <=
``loco.PIVOT_TOL`` T.G_jj: the fold alone touched the column and the subtraction left noise (``ridge_path``'s downdate
convention); its row, column and q_j are zero in exact arithmetic and are taken as zero.  The (F + 1) x Q problems (every
fold left out, and none) all start cold and are independent.  The GPU pass is ``fsnap_lasso_path`` (csrc/fsnap_lasso.hip,
K <= 144, one wave per problem); this module holds the fold dealing, the same scheme on the host (``lasso_path_host``:
``_capi.lasso_gram`` over the same downdated systems -- the route of wider systems, the baseline and the check of the
kernel; no GPU needed once the statistics are given) and the tables.
"""
from __future__ import annotations

import os
from collections import namedtuple
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from . import loco, ridge_path

MAX_K = 144                  # fsnap::LASSO_MAX_K
PIVOT_TOL = loco.PIVOT_TOL
METHODS = ("auto", "device", "host")
TABLES = ("auto", "rows", "stats")
ROWS_TABLE_MAX = 512         # table="auto": the row pass while F * Q coefficient vectors stay at or below this
HOST_THREADS = 16
CAT_STATS_MAX_BYTES = 2 << 30     # FSNAP_CAT_STATS_MAX_BYTES

LassoPath = namedtuple("LassoPath", ["alphas", "fits", "nonzeros", "sweeps", "gaps", "converged", "table", "fold_of_unit",
                                     "cv_error", "cv_se", "best", "best_alpha", "sparsest", "sparsest_alpha"])


def check_alphas(alphas):
    """The grid as a float64 vector; ValueError when it is empty or holds a negative or non-finite value."""
    alphas = np.asarray(alphas, dtype=np.float64).reshape(-1).copy()
    if alphas.size < 1:
        raise ValueError("lasso_path: the alpha grid is empty")
    if not np.all(np.isfinite(alphas)) or np.any(alphas < 0.0):
        raise ValueError("lasso_path: every alpha must be finite and >= 0")
    return alphas


def check_solver(solver):
    """ValueError unless the solver is a LASSO that does not fit through ``apply_transpose``."""
    kind = type(solver).__name__
    sec = solver.config.sections
    if kind != "LASSO":
        raise ValueError(f"lasso_path: {kind} has no LASSO path (only LASSO has; RIDGE and SVD have ridge_path)")
    if "EXTRAS" in sec and sec["EXTRAS"].apply_transpose:
        raise ValueError("lasso_path: a fit through apply_transpose has no rows to hold out (its samples are the columns of G)")


def choose_method(method, K):
    """"device" (the kernel) or "host".  "auto" takes the kernel wherever it exists (K <= 144) and the host route beyond;
    profiles/lasso_path_timing.txt records both routes at the shapes scripts/lasso_path_timing.py times."""
    if method not in METHODS:
        raise ValueError(f"lasso_path: method must be one of {', '.join(METHODS)}")
    if method == "device" and K > MAX_K:
        raise ValueError(f"lasso_path: method='device' needs K <= {MAX_K} (K = {K})")
    if method == "auto":
        return "device" if K <= MAX_K else "host"
    return method


def sorted_units(keys):
    """The distinct unit keys in sorted order (by value; by their string where the values do not compare)."""
    keys = list(dict.fromkeys(keys))
    try:
        return sorted(keys)
    except TypeError:
        return sorted(keys, key=str)


def deal_folds(keys, folds=5, seed=0):
    """({unit key: fold id}, F) for the distinct unit ``keys``.  ``folds`` as an int F: the units in sorted key order are
    shuffled by ``numpy.random.default_rng(seed)`` and dealt round-robin (deterministic, fold sizes differ by at most one
    unit); ``None``: every unit is its own fold, in sorted key order; a mapping from unit key to fold label: the folds are its
    distinct labels in sorted order."""
    keys = sorted_units(keys)
    if folds is None:
        return {k: i for i, k in enumerate(keys)}, len(keys)
    if hasattr(folds, "keys"):
        missing = [k for k in keys if k not in folds]
        if missing:
            raise ValueError(f"lasso_path: the fold mapping has no entry for unit {missing[0]!r}")
        ids = sorted_units(folds[k] for k in keys)
        pos = {v: i for i, v in enumerate(ids)}
        return {k: pos[folds[k]] for k in keys}, len(ids)
    if isinstance(folds, bool) or int(folds) != folds:
        raise ValueError("lasso_path: folds must be an int, None or a mapping from unit to fold")
    F = int(folds)
    if F < 2:
        raise ValueError(f"lasso_path: folds = {F}; at least 2 are needed to hold rows out")
    if F > len(keys):
        raise ValueError(f"lasso_path: {F} folds for {len(keys)} units")
    perm = np.random.default_rng(seed).permutation(len(keys))
    return {keys[int(u)]: i % F for i, u in enumerate(perm)}, F


def sum_blocks(blocks, nsub=1):
    """(folds, total) from the F * nsub packed blocks (rows of a 2-D array): fold f is the sum of its ``nsub`` sub-blocks, the
    total the sum of the folds, both added one by one in index order (the order of kernel S1, so the bits agree)."""
    blocks = np.asarray(blocks, dtype=np.float64)
    F = blocks.shape[0] // nsub
    folds = np.empty((F, blocks.shape[1]))
    for f in range(F):
        s = blocks[f * nsub].copy()
        for k in range(1, nsub):
            s = s + blocks[f * nsub + k]
        folds[f] = s
    total = folds[0].copy()
    for f in range(1, F):
        total = total + folds[f]
    return folds, total


def unpack(block, K):
    """(G (K x K), c (K), bb, n) of one packed block."""
    return block[:K * K].reshape(K, K), block[K * K:K * K + K], float(block[K * K + K]), float(block[K * K + K + 2])


def downdated(folds, total, f, K):
    """The system of problem f (f = F: no fold left out) as the kernel forms it: (Qm, qv, y2, n, dead) with the rows, columns
    and q entries of the dead coordinates set to zero."""
    TG, Tc, Tbb, Tn = unpack(total, K)
    if f < folds.shape[0]:
        G, c, bb, n = unpack(folds[f], K)
        Qm, qv, y2, nn = TG - G, Tc - c, Tbb - bb, Tn - n
    else:
        Qm, qv, y2, nn = TG.copy(), Tc.copy(), Tbb, Tn
    tjj = np.diag(TG)
    dead = (tjj == 0.0) | (np.diag(Qm) <= PIVOT_TOL * tjj)
    Qm[dead, :] = 0.0
    Qm[:, dead] = 0.0
    qv[dead] = 0.0
    return np.ascontiguousarray(Qm), np.ascontiguousarray(qv), y2, nn, dead


def lasso_path_host(blocks, K, alphas, max_iter, tol, nsub=1, threads=None):
    """``fsnap_lasso_path`` on the host from the downloaded ``blocks`` (F * nsub rows of K^2 + K + 3 doubles): the same
    sums, downdates and dead-column rule, ``_capi.lasso_gram`` per problem from a pool of ``threads`` Python threads
    (default: at most 16; the downdates and the wrapper's own work around every solve hold the interpreter lock, so small
    problems do not scale with the threads).
    Returns (coef ((F + 1) x Q x K), info ((F + 1) x Q x 4: sweeps, last duality gap, l1_reg, n), heldout (F x Q x 3: n_f,
    bb_f - 2 beta . c_f + beta^T G_f beta, bb_f))."""
    from .. import _capi

    alphas = check_alphas(alphas)
    folds, total = sum_blocks(blocks, nsub)
    F, Q = folds.shape[0], alphas.size
    coef = np.zeros((F + 1, Q, K))
    info = np.zeros((F + 1, Q, 4))
    held = np.zeros((F, Q, 3))
    systems = [downdated(folds, total, f, K) for f in range(F + 1)]
    dead = [bool(sy[4].all()) for sy in systems]

    def solve(p):
        f, q = divmod(p, Q)
        Qm, qv, y2, n, _ = systems[f]
        l1 = float(alphas[q]) * n
        # no live coordinate: the first sweep already is the fixed point (the kernel stops there too)
        beta, sweeps, gap = _capi.lasso_gram(Qm, qv, y2, l1, 1 if dead[f] else int(max_iter), float(tol))
        coef[f, q] = beta
        info[f, q] = (sweeps, gap, l1, n)
        if f < F:
            G, c, bb, nf = unpack(folds[f], K)
            held[f, q] = (nf, bb - 2.0 * (beta @ c) + beta @ (G @ beta), bb)

    threads = min(HOST_THREADS, os.cpu_count() or 1) if threads is None else int(threads)
    if threads > 1 and (F + 1) * Q > 1:
        with ThreadPoolExecutor(max_workers=threads) as pool:
            list(pool.map(solve, range((F + 1) * Q)))
    else:
        for p in range((F + 1) * Q):
            solve(p)
    return coef, info, held


def cv_curve(alphas, heldout):
    """(cv_error, cv_se, best, sparsest) from heldout (F x Q x 3: n_f, weighted squared error of fold f under its own refit,
    bb_f).  cv_error: the pooled weighted held-out mean squared error per alpha, sum_f sse_f / sum_f n_f; cv_se: the standard
    error over the folds that hold rows of their own mean squared errors, std(sse_f / n_f, ddof=1) / sqrt(folds) (0 with fewer
    than two); best: the grid index of the smallest cv_error, ties to the larger alpha; sparsest: the index of the largest
    alpha with cv_error <= cv_error[best] + cv_se[best] (the one-standard-error rule).  Both None when no fold holds rows."""
    alphas = np.asarray(alphas, dtype=np.float64)
    heldout = np.asarray(heldout, dtype=np.float64)
    Q = alphas.size
    n = heldout[:, :, 0]
    used = n[:, 0] > 0 if heldout.shape[0] else np.zeros(0, dtype=bool)
    if not used.any():
        return np.full(Q, np.nan), np.full(Q, np.nan), None, None
    sse, n = heldout[used, :, 1], n[used]
    cv_error = sse.sum(axis=0) / n.sum(axis=0)
    nf = sse.shape[0]
    cv_se = np.std(sse / n, axis=0, ddof=1) / np.sqrt(nf) if nf > 1 else np.zeros(Q)
    best = None
    for q in range(Q):
        if not np.isfinite(cv_error[q]):
            continue
        if best is None or cv_error[q] < cv_error[best] or (cv_error[q] == cv_error[best] and alphas[q] > alphas[best]):
            best = q
    if best is None:
        return cv_error, cv_se, None, None
    sparsest = best
    for q in range(Q):
        if np.isfinite(cv_error[q]) and cv_error[q] <= cv_error[best] + cv_se[best] and alphas[q] > alphas[sparsest]:
            sparsest = q
    return cv_error, cv_se, best, sparsest


def stats_table(alphas, heldout):
    """``table="stats"``: DataFrame indexed (alpha, Row_Type) with the ``*ALL`` row alone; ncount and w_rmse from the
    statistics form of the held-out error, mae and rmse (which need the rows) NaN."""
    from pandas import DataFrame, MultiIndex

    heldout = np.asarray(heldout, dtype=np.float64)
    n = heldout[:, :, 0].sum(axis=0)
    sse = heldout[:, :, 1].sum(axis=0)
    rows = [(int(n[q]), np.nan, np.nan, np.sqrt(max(sse[q], 0.0) / n[q]) if n[q] > 0 else np.nan) for q in range(len(alphas))]
    index = MultiIndex.from_tuples([(float(a), "*ALL") for a in alphas], names=["alpha", "Row_Type"])
    return DataFrame(rows, index=index, columns=["ncount", "mae", "rmse", "w_rmse"])


def pool_rows(sums4, counts, F, Q, nclass):
    """(Q x nclass x 4) pooled sums n, sum |r|, sum r^2, sum (w r)^2 of the held-out rows from one ``fsnap_candidate_rows``
    pass: sums4 (F Q x F nclass x 4: sum |r|, sum r^2, sum |w r|, sum (w r)^2 of vector (f, q) over category (fold, class)),
    of which only the vector's own fold is kept; counts (F nclass): rows per category.  Folds are added in index order."""
    sums4 = np.asarray(sums4, dtype=np.float64).reshape(F, Q, F, nclass, 4)
    counts = np.asarray(counts, dtype=np.float64).reshape(F, nclass)
    pooled = np.zeros((Q, nclass, 4))
    for f in range(F):
        own = sums4[f, :, f]                                   # Q x nclass x 4
        pooled[:, :, 0] += counts[f][None, :]
        pooled[:, :, 1] += own[:, :, 0]
        pooled[:, :, 2] += own[:, :, 1]
        pooled[:, :, 3] += own[:, :, 3]
    return pooled


def row_categories(units, train, fold_of_unit, row_class, nsub):
    """int32 category of every row in the layout fold x row class: fold * nsub + class (``nsub`` = number of classes; 1: the
    fold alone) for training rows, -1 for testing rows and rows off the mask, which take no part."""
    train = np.asarray(train, dtype=bool)
    fold = np.fromiter((fold_of_unit[u.item() if isinstance(u, np.generic) else u] if t else -1 for u, t in zip(units, train)),
                       dtype=np.int64, count=train.shape[0])
    cls = np.asarray(row_class, dtype=np.int64) if nsub > 1 else 0
    return np.where(fold >= 0, fold * nsub + cls, -1).astype(np.int32)


def lasso_path(solver, alphas, folds=5, by="Configs", fs_dict=None, b=None, w=None, tol=None, max_iter=None, method="auto",
               table="auto", seed=0):
    """``Solver.lasso_path``: see there."""
    from .. import _capi

    who = "lasso_path"
    pt = solver.pt
    check_solver(solver)                                    # every rank refuses alike
    alphas = check_alphas(alphas)
    if method not in METHODS:
        raise ValueError(f"lasso_path: method must be one of {', '.join(METHODS)}")
    if table not in TABLES:
        raise ValueError(f"lasso_path: table must be one of {', '.join(TABLES)}")
    fitted = np.array([1.0 if solver.last_statistics is not None else 0.0])
    if pt.multi:
        pt.allreduce_host(fitted, _capi.REDUCE_MAX)
    if not fitted[0]:
        raise RuntimeError("lasso_path: call perform_fit first")
    tol = float(type(solver).TOL if tol is None else tol)
    max_iter = int(solver.config.sections["LASSO"].max_iter if max_iter is None else max_iter)
    if not (np.isfinite(tol) and tol >= 0.0) or max_iter < 1:
        raise ValueError(f"lasso_path: tol = {tol}, max_iter = {max_iter}")
    # b and w are checked for their lengths only: the statistics and the row pass read the resident rows, truths and weights
    labels, b, w, testing, names, row_class, nclass = ridge_path.resolve_rows(solver, who, by, fs_dict, b, w)
    m, train = b.shape[0], ~testing
    ctx = pt.hip()
    K = ctx.K if m > 0 else 0
    if pt.multi:
        K = max(pt.allgather_object(int(K)))
    if m > 0 and ctx.m != m:
        raise ValueError(f"lasso_path: the resident rows ({ctx.m} x {ctx.K}) are not those of the fit ({m} rows)")
    method = choose_method(method, K)
    _, _, units = loco.unit_index(labels[by], train)
    if pt.multi:
        units = [u for part in pt.allgather_object(units) for u in part]      # a unit may span ranks
    fold_of_unit, F = deal_folds(units, folds, seed)
    Q = alphas.size
    asked = table
    if table == "auto":
        table = "rows" if F * Q <= ROWS_TABLE_MAX else "stats"
    # ONE layout, fold x row class, serves the statistics and the row pass, so both tables come from the same bits; the folds
    # alone where that many blocks would pass FSNAP_CAT_STATS_MAX_BYTES (then only the statistics table exists)
    nsub = nclass if F * nclass * (K * K + K + 3) * 8 <= CAT_STATS_MAX_BYTES else 1
    if nsub == 1 and nclass > 1:
        if asked == "rows":
            raise ValueError(f"lasso_path: table='rows' needs {F} folds x {nclass} row classes of statistics, more than "
                             "FSNAP_CAT_STATS_MAX_BYTES; use table='stats'")
        table = "stats"
    ncat = F * nsub
    cat = row_categories(labels[by], train, fold_of_unit, row_class, nsub)
    # one pass over the rows: the statistics of every (fold, row class), on every rank
    layout = ctx.cat_prepare(cat, ncat) if m > 0 else 0
    if pt.multi:
        layout, dptr = ctx.cat_normal_eq_dist(layout, K, ncat)
    else:
        dptr = ctx.cat_normal_eq(layout)
    if method == "device":
        coef, info, held = ctx.lasso_path(dptr, K, F, nsub, alphas, max_iter, tol)
    else:
        T = K * K + K + 3
        blocks = np.empty((ncat, T))
        for i in range(ncat):
            G, c, s = ctx.download_packed(dptr + i * T * 8, K)
            blocks[i, :K * K], blocks[i, K * K:K * K + K], blocks[i, K * K + K:] = G.ravel(), c, s
        coef, info, held = lasso_path_host(blocks, K, alphas, max_iter, tol, nsub)
    cv_error, cv_se, best, sparsest = cv_curve(alphas, held)
    if table == "rows":
        if m > 0:
            sums4 = ctx.candidate_rows(layout, coef[:F].reshape(F * Q, K), None, _capi.CAND_ERROR_SUMS, ncat)
            counts = np.bincount(cat[cat >= 0], minlength=ncat)
            pooled = pool_rows(sums4, counts, F, Q, nclass)
        else:
            pooled = np.zeros((Q, nclass, 4))
        if pt.multi:
            pooled = np.ascontiguousarray(pooled)
            pt.allreduce_host(pooled.reshape(-1))
        frame = ridge_path.path_table(alphas, pooled, names)
    else:
        frame = stats_table(alphas, held)
    # y2 of every problem from the folds' bb (added in index order, as the total is)
    bb = held[:, 0, 2]
    tot = bb[0]
    for f in range(1, F):
        tot = tot + bb[f]
    y2 = np.concatenate([tot - bb, [tot]])
    sweeps = info[:, :, 0].astype(np.int64)
    gaps = info[:, :, 1]
    converged = gaps < tol * y2[:, None]
    fits = coef[F].copy()
    return LassoPath(alphas, fits, np.count_nonzero(fits, axis=1), sweeps, gaps, converged, frame, fold_of_unit, cv_error, cv_se,
                     best, None if best is None else float(alphas[best]), sparsest,
                     None if sparsest is None else float(alphas[sparsest]))
