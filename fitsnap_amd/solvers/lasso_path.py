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
K <= 144, one wave per problem); this module holds the same scheme on the host (``lasso_path_host``: ``_capi.lasso_gram``
over the same downdated systems -- the route of wider systems, the baseline and the check of the kernel; no GPU needed once
the statistics are given) and the picks.  Fold dealing, block sums, downdates and tables are the fold frame's (``folds``;
DESIGN.md, "The fold frame"); its names stay importable from here.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from . import folds as fold_frame, ridge_path
from .folds import (CAT_STATS_MAX_BYTES, HOST_THREADS, METHODS, PIVOT_TOL, ROWS_TABLE_MAX, TABLES, cv_curve,  # noqa: F401
                    deal_folds, downdated, download_blocks, pool_rows, row_categories, sorted_units, stats_table, sum_blocks, unpack)

MAX_K = 144                  # fsnap::LASSO_MAX_K

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

    fold_frame.run_pool(solve, (F + 1) * Q, threads)
    return coef, info, held


def lasso_path(solver, alphas, folds=5, by="Configs", fs_dict=None, b=None, w=None, tol=None, max_iter=None, method="auto",
               table="auto", seed=0):
    """``Solver.lasso_path``: see there."""
    who = "lasso_path"
    check_solver(solver)                                    # every rank refuses alike
    alphas = check_alphas(alphas)
    if method not in METHODS:
        raise ValueError(f"lasso_path: method must be one of {', '.join(METHODS)}")
    if table not in TABLES:
        raise ValueError(f"lasso_path: table must be one of {', '.join(TABLES)}")
    fold_frame.check_fitted(solver, who)
    tol = float(type(solver).TOL if tol is None else tol)
    max_iter = int(solver.config.sections["LASSO"].max_iter if max_iter is None else max_iter)
    if not (np.isfinite(tol) and tol >= 0.0) or max_iter < 1:
        raise ValueError(f"lasso_path: tol = {tol}, max_iter = {max_iter}")
    fr = fold_frame.resolve(solver, who, by, fs_dict, b, w)
    K, Q = fr.K, alphas.size
    method = choose_method(method, K)
    fold_of_unit, F = fold_frame.deal_units(fr.pt, fr.labels, fr.train, folds, seed)
    table, nsub = fold_frame.plan_table(who, table, F, Q, fr.nclass, K)
    fold_frame.statistics(fr, fold_of_unit, F, nsub)
    if method == "device":
        coef, info, held = fr.ctx.lasso_path(fr.dptr, K, F, nsub, alphas, max_iter, tol)
    else:
        coef, info, held = lasso_path_host(download_blocks(fr.ctx, fr.dptr, fr.ncat, K), K, alphas, max_iter, tol, nsub)
    cv_error, cv_se, best, sparsest = cv_curve(alphas, held)
    if table == "rows":
        frame = ridge_path.path_table(alphas, fold_frame.rows_pooled(fr, coef[:F], F, Q), fr.names)
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
