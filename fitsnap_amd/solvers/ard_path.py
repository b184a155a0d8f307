"""Grouped K-fold ARD threshold paths: which ``[ARD]`` setting (``logcut``, ``scap``, ``scai``; under ``directmethod``
``threshold_lambda``, ``alphabig``, ``lambdasmall``) predicts held-out units best, and how many descriptors it keeps.

Every iteration of ``ARD._ard_loop`` touches the weighted training rows only through (X^T X, X^T y, |y|^2, sum y, n).  With
the units dealt into F folds and one packed block [G_f | c_f | bb_f, sum wb_f, n_f] per fold -- ONE pass over the rows, the
layout and statistics of the fold frame --, problem (f, q) is the ARD fit of setting q on "total minus block f" (f = F: on all
training rows):

    Qm = T.G - G_f,  qv = T.c - c_f,  y2 = T.bb - bb_f,  s = T.sum wb - sum wb_f,  n = T.n - n_f
    dead_j: T.G_jj == 0 or Qm_jj <= loco.PIVOT_TOL T.G_jj  -> never kept, coefficient 0
    var = y2 / n - (s / n)^2,  ap = 1 / var,  alpha_init = 1 / (var + eps)
    alpha_1 = alpha_2 = scap ap,  lambda_1 = lambda_2 = scai ap,  threshold_lambda = 10^(int(|log10 ap|) + logcut)
    (directmethod: alpha_1 = alpha_2 = alphabig, lambda_1 = lambda_2 = lambdasmall, threshold_lambda as given)

the hyper-parameters ``ARD.perform_fit`` would compute on the rows that remain, followed by ``ARD._ard_loop`` statement for
statement.  Two deliberate differences from ``ARD.perform_fit``: the residual sum of squares of an iteration is the
statistics form max(y2 - 2 coef . qv + coef^T Qm coef, 0) (there are no rows per fold to stream; 3e-9 ... 7e-9 in the
coefficients on the Ta rows), and on the GPU the inverse comes from a Cholesky factor of the equilibrated matrix instead of
``pinvh`` (the matrix is positive definite whenever every lambda is positive; 1e-9 ... 4e-9 on the Ta rows).  A non-positive
pivot or a non-finite lambda ends a problem with status 1 and NaN coefficients; a problem whose remaining rows have n <= 0 or
var <= 0 gets status 1 without being run.

The GPU pass is ``fsnap_ard_path`` (csrc/fsnap_ard.hip, K <= 144, one workgroup per problem); this module holds the grid, the
hyper-parameters, the same scheme on the host (``ard_path_host``: ``ARD._ard_loop`` over the same downdated systems -- the
route of wider systems, the baseline and the check of the kernel; no GPU needed once the statistics are given) and the
picks.  Fold dealing, block sums, downdates and tables are the fold frame's (``folds``; DESIGN.md, "The fold frame").
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from . import folds as fold_frame, ridge_path
from .._hostblas import blas_threads
from .folds import TABLES, cv_curve, downdated, download_blocks, stats_table, sum_blocks, unpack

MAX_K = 144                  # fsnap::ARD_MAX_K
METHODS = ("auto", "device", "host")
KEYS = ("logcut", "scap", "scai")
KEYS_DIRECT = ("threshold_lambda", "alphabig", "lambdasmall")
NHYPER = 6                   # alpha_1, alpha_2, lambda_1, lambda_2, threshold_lambda, alpha_init
NINFO = 6                    # iterations, kept, final alpha_, last sum |d coef|, smallest pivot, status
VOID_HYPER = (0.0, 0.0, 0.0, 0.0, 1.0, 1.0)      # what a problem that is not run carries through the entry point

ArdPath = namedtuple("ArdPath", ["grid", "fits", "lambdas", "nonzeros", "iterations", "status", "alpha_", "table",
                                 "fold_of_unit", "cv_error", "cv_se", "best", "best_setting", "sparsest", "sparsest_setting"])


def check_solver(solver):
    """ValueError unless the solver is an ARD that does not fit through ``apply_transpose``."""
    kind = type(solver).__name__
    sec = solver.config.sections
    if kind != "ARD":
        raise ValueError(f"ard_path: {kind} has no ARD path (only ARD has; LASSO has lasso_path, RIDGE and SVD have ridge_path)")
    if "EXTRAS" in sec and sec["EXTRAS"].apply_transpose:
        raise ValueError("ard_path: a fit through apply_transpose has no rows to hold out (its samples are the columns of G)")


def choose_method(method, K):
    """"device" (the kernel) or "host".  "auto" takes the kernel wherever it exists (K <= 144) and the host route beyond;
    profiles/ard_path_timing.txt records both routes at the shapes scripts/ard_path_timing.py times."""
    if method not in METHODS:
        raise ValueError(f"ard_path: method must be one of {', '.join(METHODS)}")
    if method == "device" and K > MAX_K:
        raise ValueError(f"ard_path: method='device' needs K <= {MAX_K} (K = {K})")
    if method == "auto":
        return "device" if K <= MAX_K else "host"
    return method


def resolve_grid(grid, section):
    """The grid as a list of complete mappings.  Every entry overrides keys of the ``[ARD]`` section: ``logcut``, ``scap``,
    ``scai``, or under ``directmethod`` ``threshold_lambda``, ``alphabig``, ``lambdasmall``; a bare number stands for
    ``logcut`` (``threshold_lambda`` under ``directmethod``).  ValueError for an empty grid, a key of the other mode or an
    unknown one, a value that is not finite, a negative ``scap`` / ``scai`` / ``alphabig`` / ``lambdasmall`` or a
    ``threshold_lambda`` <= 0."""
    direct = bool(section.directmethod)
    keys = KEYS_DIRECT if direct else KEYS
    if hasattr(grid, "keys") or isinstance(grid, (str, bytes)) or not hasattr(grid, "__iter__"):
        raise ValueError("ard_path: the grid must be a sequence of mappings or of numbers")
    out = []
    for entry in grid:
        if not hasattr(entry, "keys"):
            entry = {keys[0]: entry}
        unknown = [k for k in entry if k not in keys]
        if unknown:
            raise ValueError(f"ard_path: unknown grid key {unknown[0]!r} ({'directmethod: ' if direct else ''}{', '.join(keys)})")
        full = {k: float(entry[k]) if k in entry else float(getattr(section, k)) for k in keys}
        for k, v in full.items():
            if not np.isfinite(v) or (k != "logcut" and v < 0.0) or (k == "threshold_lambda" and v <= 0.0):
                raise ValueError(f"ard_path: grid value {k} = {v}")
        out.append(full)
    if not out:
        raise ValueError("ard_path: the grid is empty")
    return out


def hyper_of(y2, swb, n, setting, direct):
    """(alpha_1, alpha_2, lambda_1, lambda_2, threshold_lambda, alpha_init) as ``ARD.perform_fit`` computes them from the rows
    with sum (w b)^2 = y2, sum w b = swb and count n; None when n <= 0 or the variance is not positive."""
    if not n > 0.0:
        return None
    var = y2 / n - (swb / n) ** 2
    if not (var > 0.0 and np.isfinite(var)):
        return None
    ap = 1.0 / var
    alpha_init = 1.0 / (var + np.finfo(np.float64).eps)
    if direct:
        return (setting["alphabig"], setting["alphabig"], setting["lambdasmall"], setting["lambdasmall"],
                setting["threshold_lambda"], alpha_init)
    thr = 10 ** (int(np.abs(np.log10(ap))) + setting["logcut"])
    if not (np.isfinite(thr) and thr > 0.0):
        return None
    return (setting["scap"] * ap, setting["scap"] * ap, ap * setting["scai"], ap * setting["scai"], thr, alpha_init)


def fold_hypers(folds, total, K, grid, direct):
    """(hyper ((F + 1) x Q x 6), run ((F + 1) x Q bool)) of every problem from the downdated scalars; a problem that cannot be
    posed (``hyper_of`` is None) has run = False and carries ``VOID_HYPER``."""
    F, Q, at = folds.shape[0], len(grid), K * K + K
    hyper = np.empty((F + 1, Q, NHYPER))
    run = np.ones((F + 1, Q), dtype=bool)
    for f in range(F + 1):
        y2, swb, n = (total[at + i] - folds[f, at + i] if f < F else total[at + i] for i in range(3))
        for q, setting in enumerate(grid):
            h = hyper_of(float(y2), float(swb), float(n), setting, direct)
            run[f, q] = h is not None
            hyper[f, q] = VOID_HYPER if h is None else h
    return hyper, run


def void_problems(run, coef, lam, info, held):
    """Status 1 for the problems that were not run: NaN coefficients, lambdas and held-out error, zero iterations."""
    for f, q in zip(*np.nonzero(~run)):
        coef[f, q], lam[f, q] = np.nan, np.nan
        info[f, q] = (0.0, 0.0, np.nan, np.nan, np.nan, 1.0)
        if f < held.shape[0]:
            held[f, q, 1] = np.nan


def ard_path_host(blocks, K, hyper, max_iter, tol, nsub=1, threads=None, run=None):
    """``fsnap_ard_path`` on the host from the downloaded ``blocks`` (F * nsub rows of K^2 + K + 3 doubles): the same sums,
    downdates and dead-column rule, ``ARD._ard_loop`` per problem (``pinvh`` of the equilibrated matrix; the statistics form of
    the residual sum of squares) from a pool of ``threads`` Python threads (default: at most 16).  ``run`` ((F + 1) x Q bool,
    default all): the problems to run; the others are left to ``void_problems``.
    Returns (coef ((F + 1) x Q x K), lambdas (the same shape), info ((F + 1) x Q x 6: iterations, kept columns, final alpha_,
    last sum |coef_old - coef|, smallest Cholesky pivot of the scaled matrices, status 0 converged or emptied / 1 failed / 2
    max_iter reached), heldout (F x Q x 3: n_f, bb_f - 2 beta . c_f + beta^T G_f beta, bb_f))."""
    from .ard import ARD

    hyper = np.asarray(hyper, dtype=np.float64)
    folds, total = sum_blocks(blocks, nsub)
    F, Q = folds.shape[0], hyper.shape[1]
    if hyper.shape != (F + 1, Q, NHYPER):
        raise ValueError(f"ard_path: hyper has shape {hyper.shape}, not {(F + 1, Q, NHYPER)}")
    coef = np.zeros((F + 1, Q, K))
    lam = np.ones((F + 1, Q, K))
    info = np.zeros((F + 1, Q, NINFO))
    held = np.zeros((F, Q, 3))
    systems = [downdated(folds, total, f, K) for f in range(F + 1)]

    def solve(p):
        f, q = divmod(p, Q)
        Qm, qv, y2, n, dead = systems[f]
        if f < F:
            G, c, bb, nf = unpack(folds[f], K)
            held[f, q] = (nf, 0.0, bb)
        if run is not None and not run[f, q]:
            return
        a1, a2, l1, l2, thr, a0 = (float(x) for x in hyper[f, q])
        loop = ARD.__new__(ARD)                 # the loop alone: no config, no rows (one object per problem: threads)
        loop.exact_sse = False
        probe = {}
        beta = loop._ard_loop(Qm, qv, y2, n, None, a1, a2, l1, l2, thr,
                              host_sse=lambda b: max(float(y2 - 2.0 * (b @ qv) + b @ (Qm @ b)), 0.0),
                              live=~dead, tol=float(tol), max_iter=int(max_iter), alpha_init=a0, probe=probe)
        keep = (loop.lambda_ < thr) & ~dead
        coef[f, q], lam[f, q] = beta, loop.lambda_
        if probe["status"] == 1:
            lam[f, q] = np.nan
        info[f, q] = (loop.n_iter_, keep.sum() if probe["status"] != 1 else 0, loop.alpha_, probe["delta"], probe["pivot"],
                      probe["status"])
        if f < F:
            held[f, q, 1] = bb - 2.0 * (beta @ c) + beta @ (G @ beta)

    # one limit of the BLAS pools around all problems: the loop's own limits then nest inside it, and whatever order the
    # threads leave theirs in, the pools get their size back here
    with blas_threads(K):
        fold_frame.run_pool(solve, (F + 1) * Q, threads)
    return coef, lam, info, held


def pick(cv_error, cv_se, nonzeros):
    """(best, sparsest).  best: the index of the smallest finite cv_error, ties to fewer non-zeros of the all-rows fit, then
    to the lower index; sparsest: the fewest non-zeros among the settings with cv_error <= cv_error[best] + cv_se[best], ties to
    the lower index.  (None, None) when no cv_error is finite."""
    best = None
    for q in range(len(cv_error)):
        if not np.isfinite(cv_error[q]):
            continue
        if best is None or cv_error[q] < cv_error[best] or (cv_error[q] == cv_error[best] and nonzeros[q] < nonzeros[best]):
            best = q
    if best is None:
        return None, None
    bar = cv_error[best] + (cv_se[best] if np.isfinite(cv_se[best]) else 0.0)
    sparsest = best
    for q in range(len(cv_error)):
        if np.isfinite(cv_error[q]) and cv_error[q] <= bar and (nonzeros[q] < nonzeros[sparsest]
                                                               or (nonzeros[q] == nonzeros[sparsest] and q < sparsest)):
            sparsest = q
    return best, sparsest


def cv_picks(heldout, status, nonzeros):
    """(cv_error, cv_se, best, sparsest) from heldout (F x Q x 3), status ((F + 1) x Q) and the non-zero counts of the all-rows
    fits: ``folds.cv_curve``'s pooled error and standard error, NaN for a setting with a status-1 problem, and ``pick``."""
    Q = heldout.shape[1]
    cv_error, cv_se, _, _ = cv_curve(np.arange(Q, dtype=np.float64), heldout)
    failed = (np.asarray(status) == 1).any(axis=0)
    cv_error = np.where(failed, np.nan, cv_error)
    cv_se = np.where(failed, np.nan, cv_se)
    return (cv_error, cv_se) + pick(cv_error, cv_se, nonzeros)


def setting_index(frame):
    """A fold-frame table keyed by the position in the grid: index (setting, Row_Type)."""
    frame.index = frame.index.set_levels(frame.index.levels[0].astype(np.int64), level=0).set_names(["setting", "Row_Type"])
    return frame


def ard_path(solver, grid, folds=5, by="Configs", fs_dict=None, b=None, w=None, tol=None, max_iter=None, method="auto",
             table="auto", seed=0):
    """``Solver.ard_path``: see there."""
    who = "ard_path"
    check_solver(solver)                                    # every rank refuses alike
    section = solver.config.sections["ARD"]
    direct = bool(section.directmethod)
    grid = resolve_grid(grid, section)
    if method not in METHODS:
        raise ValueError(f"ard_path: method must be one of {', '.join(METHODS)}")
    if table not in TABLES:
        raise ValueError(f"ard_path: table must be one of {', '.join(TABLES)}")
    fold_frame.check_fitted(solver, who)
    tol = float(type(solver).TOL if tol is None else tol)
    max_iter = int(type(solver).MAX_ITER if max_iter is None else max_iter)
    if not (np.isfinite(tol) and tol >= 0.0) or max_iter < 1:
        raise ValueError(f"ard_path: tol = {tol}, max_iter = {max_iter}")
    fr = fold_frame.resolve(solver, who, by, fs_dict, b, w)
    K, Q = fr.K, len(grid)
    method = choose_method(method, K)
    fold_of_unit, F = fold_frame.deal_units(fr.pt, fr.labels, fr.train, folds, seed)
    table, nsub = fold_frame.plan_table(who, table, F, Q, fr.nclass, K)
    fold_frame.statistics(fr, fold_of_unit, F, nsub)
    # the scalars (bb, sum wb, n) of the blocks decide the hyper-parameters of every problem, on either route
    blocks = download_blocks(fr.ctx, fr.dptr, fr.ncat, K)
    hyper, run = fold_hypers(*sum_blocks(blocks, nsub), K, grid, direct)
    if method == "device":
        coef, lam, info, held = fr.ctx.ard_path(fr.dptr, K, F, nsub, hyper, max_iter, tol)
    else:
        coef, lam, info, held = ard_path_host(blocks, K, hyper, max_iter, tol, nsub, run=run)
    void_problems(run, coef, lam, info, held)
    status = info[:, :, 5].astype(np.int64)
    fits = coef[F].copy()
    nonzeros = np.count_nonzero(np.nan_to_num(fits), axis=1)
    cv_error, cv_se, best, sparsest = cv_picks(held, status, nonzeros)
    index = np.arange(Q, dtype=np.float64)
    if table == "rows":
        # a failed refit's NaN vector would poison its rows' sums only; they are reported as they come
        pooled = fold_frame.rows_pooled(fr, np.nan_to_num(coef[:F]), F, Q)
        pooled[(status == 1).any(axis=0), :, 1:] = np.nan
        frame = ridge_path.path_table(index, pooled, fr.names)
    else:
        frame = stats_table(index, held)
    return ArdPath(grid, fits, lam[F].copy(), nonzeros, info[:, :, 0].astype(np.int64), status, info[:, :, 2].copy(),
                   setting_index(frame), fold_of_unit, cv_error, cv_se, best, None if best is None else grid[best], sparsest,
                   None if sparsest is None else grid[sparsest])
