"""The fold frame of the grouped K-fold paths ("The fold frame").

A path refits on "total minus fold" statistics: the units (configurations, or any label such as a group) are dealt into F
folds, ONE pass over the rows -- ``fsnap_cat_prepare`` + ``fsnap_cat_normal_eq`` with category = fold x row class -- leaves
one packed block [G_f | c_f | bb_f, sum wb, n_f] per category, and the training system of fold f is

    Qm = T.G - G_f,  qv = T.c - c_f,  y2 = T.bb - bb_f,  n = T.n - n_f                  (f = F: the total alone)

with coordinate j DEAD -- skipped, coefficient 0 -- when T.G_jj == 0 or Qm_jj <= ``loco.PIVOT_TOL`` T.G_jj (the fold alone
touched the column and the subtraction left noise).  Every refit leaves the held-out record (n_f, bb_f - 2 beta . c_f +
beta^T G_f beta, bb_f), from which the cross-validation curve and the tables follow.  This module owns all of that: the host
algebra (``deal_folds`` ... ``row_categories``, what the kernels' shared statements in csrc/fsnap_fold_body.h compute) and the
steps of a driver in the order every rank takes them (``check_fitted``, ``resolve``, ``deal_units``, ``plan_table``,
``statistics``, ``rows_pooled``; ``run_pool`` for the host routes).  ``lasso_path``, ``ard_path`` and ``omp_path`` supply their
per-problem solver, their picks and their result; ``candidates_cv`` deals its folds here.
"""
from __future__ import annotations

import os
from concurrent.futures import ThreadPoolExecutor
from types import SimpleNamespace

import numpy as np

from . import loco, ridge_path

PIVOT_TOL = loco.PIVOT_TOL
METHODS = ("auto", "device", "host")
TABLES = ("auto", "rows", "stats")
ROWS_TABLE_MAX = 512         # table="auto": the row pass while F * Q coefficient vectors stay at or below this
HOST_THREADS = 16
CAT_STATS_MAX_BYTES = 2 << 30     # FSNAP_CAT_STATS_MAX_BYTES


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


def download_blocks(ctx, dptr, ncat, K):
    """The ``ncat`` packed blocks at the device address ``dptr`` as rows of an array."""
    T = K * K + K + 3
    blocks = np.empty((ncat, T))
    for i in range(ncat):
        G, c, s = ctx.download_packed(dptr + i * T * 8, K)
        blocks[i, :K * K], blocks[i, K * K:K * K + K], blocks[i, K * K + K:] = G.ravel(), c, s
    return blocks


# ---- the steps of a driver, in the order every rank takes them (each collective is named) -------------------------------------

def check_fitted(solver, who):
    """RuntimeError on every rank unless some rank holds the statistics of a fit (collective: one all-reduce)."""
    from .. import _capi

    fitted = np.array([1.0 if solver.last_statistics is not None else 0.0])
    if solver.pt.multi:
        solver.pt.allreduce_host(fitted, _capi.REDUCE_MAX)
    if not fitted[0]:
        raise RuntimeError(f"{who}: call perform_fit first")


def resolve(solver, who, by, fs_dict, b, w):
    """The rows of the last fit as a frame record: pt, ctx, m (local rows), K (agreed across the ranks), labels (the unit label
    of every row), train (mask), names (sorted Row_Type names), row_class, nclass.  ``b`` and ``w`` are checked for their
    lengths only: the statistics and the row pass read the resident rows, truths and weights.  ValueError when the resident
    rows are not those of the fit.  Collective: ``resolve_rows``' all-gather of the names, then one of K."""
    pt = solver.pt
    labels, b, w, testing, names, row_class, nclass = ridge_path.resolve_rows(solver, who, by, fs_dict, b, w)
    m = b.shape[0]
    ctx = pt.hip()
    K = ctx.K if m > 0 else 0
    if pt.multi:
        K = max(pt.allgather_object(int(K)))
    if m > 0 and ctx.m != m:
        raise ValueError(f"{who}: the resident rows ({ctx.m} x {ctx.K}) are not those of the fit ({m} rows)")
    return SimpleNamespace(pt=pt, ctx=ctx, m=m, K=K, labels=labels[by], train=~testing, names=names, row_class=row_class,
                           nclass=nclass)


def deal_units(pt, labels, train, folds, seed):
    """(fold_of_unit, F): the units of the training rows, gathered over the ranks (a unit may span ranks; collective: one
    all-gather), dealt by ``deal_folds`` -- the same folds on every rank."""
    _, _, units = loco.unit_index(labels, train)
    if pt.multi:
        units = [u for part in pt.allgather_object(units) for u in part]
    return deal_folds(units, folds, seed)


def plan_table(who, table, F, Q, nclass, K):
    """(table, nsub).  ``table="auto"`` is the row pass while F * Q coefficient vectors stay at or below ``ROWS_TABLE_MAX``.
    ONE layout, fold x row class (nsub = nclass), serves the statistics and the row pass, so both tables come from the same
    bits; the folds alone (nsub = 1) where that many blocks would pass FSNAP_CAT_STATS_MAX_BYTES -- then only the statistics
    table exists, and an explicit ``table="rows"`` is a ValueError."""
    asked = table
    if table == "auto":
        table = "rows" if F * Q <= ROWS_TABLE_MAX else "stats"
    nsub = nclass if F * nclass * (K * K + K + 3) * 8 <= CAT_STATS_MAX_BYTES else 1
    if nsub == 1 and nclass > 1:
        if asked == "rows":
            raise ValueError(f"{who}: table='rows' needs {F} folds x {nclass} row classes of statistics, more than "
                             "FSNAP_CAT_STATS_MAX_BYTES; use table='stats'")
        table = "stats"
    return table, nsub


def statistics(frame, fold_of_unit, F, nsub):
    """One pass over the rows: the statistics of every (fold, row class), on every rank.  Adds to the frame cat (category per
    row), ncat = F * nsub, layout and dptr (the device address of the ncat packed blocks).  Collective on several ranks."""
    ctx = frame.ctx
    frame.ncat = F * nsub
    frame.cat = row_categories(frame.labels, frame.train, fold_of_unit, frame.row_class, nsub)
    frame.layout = ctx.cat_prepare(frame.cat, frame.ncat) if frame.m > 0 else 0
    if frame.pt.multi:
        frame.layout, frame.dptr = ctx.cat_normal_eq_dist(frame.layout, frame.K, frame.ncat)
    else:
        frame.dptr = ctx.cat_normal_eq(frame.layout)
    return frame


def rows_pooled(frame, coef, F, Q):
    """(Q x nclass x 4) sums n, sum |r|, sum r^2, sum (w r)^2 of every row under the refit ``coef[f, q]`` (F x Q x K) that held
    its fold out: one ``fsnap_candidate_rows`` pass over the layout of ``statistics``, ``pool_rows``, and on several ranks one
    all-reduce (collective)."""
    from .. import _capi

    if frame.m > 0:
        sums4 = frame.ctx.candidate_rows(frame.layout, coef.reshape(F * Q, frame.K), None, _capi.CAND_ERROR_SUMS, frame.ncat)
        counts = np.bincount(frame.cat[frame.cat >= 0], minlength=frame.ncat)
        pooled = pool_rows(sums4, counts, F, Q, frame.nclass)
    else:
        pooled = np.zeros((Q, frame.nclass, 4))
    if frame.pt.multi:
        pooled = np.ascontiguousarray(pooled)
        frame.pt.allreduce_host(pooled.reshape(-1))
    return pooled


def run_pool(solve, n, threads=None):
    """``solve(i)`` for every i in range(n), from a pool of ``threads`` Python threads (default: at most ``HOST_THREADS``);
    one after the other with one thread or one problem."""
    threads = min(HOST_THREADS, os.cpu_count() or 1) if threads is None else int(threads)
    if threads > 1 and n > 1:
        with ThreadPoolExecutor(max_workers=threads) as pool:
            list(pool.map(solve, range(n)))
    else:
        for i in range(n):
            solve(i)
