"""Grouped K-fold greedy sparse-selection paths: orthogonal matching pursuit and its orthogonal-least-squares form.

"The best s of my K basis functions, and which s": forward selection hands out a nested, ordered list of columns with the
UNSHRUNK least-squares fit at every size.  It touches the weighted training rows only through (X^T X, X^T y, |y|^2), so with
the units dealt into F folds and one packed block per fold -- the fold frame's ONE pass over the rows, category = fold x row
class -- the training system of fold f is "total minus block f":

    Qm = T.G - G_f,  qv = T.c - c_f,  y2 = T.bb - bb_f                                  (f = F: the total alone)

and the F + 1 problems are independent.  The recurrence is a Cholesky factorisation of Qm whose pivot is chosen by the
criterion, with the right-hand side carried along (``fsnap_omp_gram``, include/fsnap_hip.h, states it in full):

    state    t_j = Qm_jj, r_j = qv_j, e_0 = y2; a column is DEAD when T.G_jj == 0 or Qm_jj <= PIVOT_TOL T.G_jj
    step s   candidates: live, not chosen, not struck (t_j <= PIVOT_TOL Qm_jj strikes a column for good);
             the next forced column if it is a candidate, else argmax r_j^2 / Qm_jj ("omp") or r_j^2 / t_j ("ols"), ties to
             the lowest index; l = sqrt(t_j*), w_k = (Qm_{j*,k} - sum_u W_uj* W_uk) / l, z_s = r_j* / l, r_k -= w_k z_s,
             t_k -= w_k^2, e_s = e_{s-1} - z_s^2
    beta_s   L^T beta = z_{1..s} on the support, L[v][u] = W_{u,j_v}; zero elsewhere
    held out h_{f,s} = bb_f - 2 beta . c_f + beta^T G_f beta

"omp" is scikit-learn's ``orthogonal_mp_gram`` on the column-normalised system; "ols" is forward stepwise regression (the
column that lowers the residual most).  The GPU pass is ``fsnap_omp_path`` (csrc/fsnap_omp.hip, K <= 144, at most 128 steps,
one wave per problem); this module holds the same scheme on the host (``omp_path_host``: ``_capi.omp_gram`` over the same
downdated systems -- the route of wider systems, the baseline and the check of the kernel; no GPU needed once the statistics
are given), the picks and the tables.  Fold dealing, block sums, downdates and tables are the fold frame's (``folds``;
DESIGN.md, "The fold frame").
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from . import folds as fold_frame, ridge_path
from .folds import METHODS, TABLES, cv_curve, downdated, download_blocks, sum_blocks, unpack

MAX_K = 144                  # fsnap::OMP_MAX_K
MAX_STEPS = 128              # fsnap::OMP_MAX_S: the factor rows of a problem stay in one CU's LDS
CRITERIA = ("omp", "ols")

OmpPath = namedtuple("OmpPath", ["terms", "order", "fold_orders", "levels", "fits", "train_sse", "table", "fold_of_unit",
                                 "cv_error", "cv_se", "best", "best_terms", "sparsest", "sparsest_terms", "frequency"])


def check_solver(solver):
    """ValueError unless the solver is an OMP that does not fit through ``apply_transpose``."""
    kind = type(solver).__name__
    sec = solver.config.sections
    if kind != "OMP":
        raise ValueError(f"omp_path: {kind} has no selection path (only OMP has; LASSO has lasso_path, ARD has ard_path, RIDGE "
                         "and SVD have ridge_path)")
    if "EXTRAS" in sec and sec["EXTRAS"].apply_transpose:
        raise ValueError("omp_path: a fit through apply_transpose has no rows to hold out (its samples are the columns of G)")


def check_criterion(criterion):
    if not isinstance(criterion, str) or criterion.lower() not in CRITERIA:
        raise ValueError(f"omp_path: criterion must be one of {', '.join(CRITERIA)}")
    return criterion.lower()


def check_forced(forced, K):
    """The forced columns as an int32 vector; ValueError for an index outside 0 ... K - 1 or a repeated one."""
    forced = np.asarray(() if forced is None else forced, dtype=np.int64).reshape(-1)
    if forced.size and (forced.min() < 0 or forced.max() >= K or np.unique(forced).size != forced.size):
        raise ValueError(f"omp_path: forced = {forced.tolist()}: distinct column indices in 0 ... {K - 1}")
    return forced.astype(np.int32)


def default_levels(S):
    """A short geometric ladder 1, 2, 3, 4, 6, 8, 12, 16, ... up to and including S."""
    out, a = {int(S)}, 1
    while a < S:
        out.add(a)
        if a + a // 2 < S and a >= 2:
            out.add(a + a // 2)
        a *= 2
    return np.array(sorted(out), dtype=np.int32)


def check_levels(levels, S):
    """The levels as a sorted int32 vector of distinct values in 1 ... S (None: ``default_levels``)."""
    if levels is None:
        return default_levels(S)
    lv = np.asarray(levels, dtype=np.int64).reshape(-1)
    if lv.size < 1 or lv.min() < 1 or lv.max() > S:
        raise ValueError(f"omp_path: levels must lie in 1 ... {S}")
    return np.unique(lv).astype(np.int32)


def choose_method(method, K, S):
    """"device" (the kernel) or "host".  "auto" takes the kernel wherever it exists (K <= 144, at most 128 steps) and the host
    route beyond: one problem is a wave's serial recurrence, some 16 times slower than on a host core, but the F + 1
    problems run side by side and the statistics need not come back, which already wins at F = 5
    (profiles/omp_path_timing.txt records both routes at the shapes scripts/omp_path_timing.py times)."""
    if method not in METHODS:
        raise ValueError(f"omp_path: method must be one of {', '.join(METHODS)}")
    fits = K <= MAX_K and S <= MAX_STEPS
    if method == "device" and not fits:
        raise ValueError(f"omp_path: method='device' needs K <= {MAX_K} and max_terms <= {MAX_STEPS} (K = {K}, max_terms = {S})")
    if method == "auto":
        return "device" if fits else "host"
    return method


def omp_path_host(blocks, K, criterion, forced, S, levels, nsub=1, threads=None):
    """``fsnap_omp_path`` on the host from the downloaded ``blocks`` (F * nsub rows of K^2 + K + 3 doubles): the same sums,
    downdates and dead-column rule, ``_capi.omp_gram`` per problem from a pool of ``threads`` Python threads (default: at
    most 16; the library call releases the interpreter lock).  Any K, any S <= K.
    Returns (order ((F + 1) x S), path ((F + 1) x S x 3: e_s, score, pivot), heldout (F x S x 3: n_f, bb_f - 2 beta . c_f +
    beta^T G_f beta after s steps, bb_f), coef ((F + 1) x Q x K at the levels))."""
    from .. import _capi

    criterion = check_criterion(criterion)
    forced = check_forced(forced, K)
    levels = check_levels(levels, S)
    folds, total = sum_blocks(blocks, nsub)
    F, Q = folds.shape[0], levels.size
    order = np.full((F + 1, S), -1, dtype=np.int32)
    path = np.zeros((F + 1, S, 3))
    held = np.zeros((F, S, 3))
    coef = np.zeros((F + 1, Q, K))
    tdiag = np.ascontiguousarray(np.diag(unpack(total, K)[0]))

    def solve(f):
        Qm, qv, y2, _, _ = downdated(folds, total, f, K)
        o, p, beta = _capi.omp_gram(Qm, qv, y2, S, criterion, forced, tdiag)
        order[f], path[f], coef[f] = o, p, beta[levels - 1]
        if f < F:
            G, c, bb, nf = unpack(folds[f], K)
            held[f, :, 0], held[f, :, 2] = nf, bb
            held[f, :, 1] = bb - 2.0 * (beta @ c) + np.einsum("sk,sk->s", beta @ G, beta)

    fold_frame.run_pool(solve, F + 1, threads)
    return order, path, held, coef


def cv_picks(terms, heldout):
    """(cv_error, cv_se, best, sparsest) over every step from heldout (F x S x 3): ``folds.cv_curve`` with the sizes
    counted downwards, so that ``best`` is the smallest pooled held-out error with ties to FEWER terms and ``sparsest`` the
    fewest terms within one standard error of it.  Indices into ``terms``; both None when no fold holds rows."""
    return cv_curve(-np.asarray(terms, dtype=np.float64), heldout)


def selection_frequency(fold_orders, best_terms, K):
    """Per column, the share of the folds' refits that chose it within their first ``best_terms`` steps (zeros without a
    pick)."""
    fold_orders = np.asarray(fold_orders)
    freq = np.zeros(K)
    if best_terms is None or fold_orders.shape[0] == 0:
        return freq
    for o in fold_orders:
        chosen = o[:best_terms]
        freq[chosen[chosen >= 0]] += 1.0
    return freq / fold_orders.shape[0]


def keyed_by_terms(frame):
    frame.index = frame.index.set_names(["terms", "Row_Type"])
    return frame


def stats_table(levels, heldout):
    """``table="stats"``: DataFrame indexed (terms, Row_Type) with the ``*ALL`` row alone; ncount and w_rmse from the
    statistics form of the held-out error at the levels, mae and rmse (which need the rows) NaN."""
    levels = np.asarray(levels, dtype=np.int64)
    return keyed_by_terms(fold_frame.stats_table(levels.astype(np.float64), np.asarray(heldout)[:, levels - 1]))


def omp_path(solver, max_terms, levels=None, criterion="ols", forced=(), folds=5, by="Configs", fs_dict=None, b=None, w=None,
             method="auto", table="auto", seed=0):
    """``Solver.omp_path``: see there."""
    who = "omp_path"
    check_solver(solver)                                    # every rank refuses alike
    criterion = check_criterion(criterion)
    if method not in METHODS:
        raise ValueError(f"omp_path: method must be one of {', '.join(METHODS)}")
    if table not in TABLES:
        raise ValueError(f"omp_path: table must be one of {', '.join(TABLES)}")
    fold_frame.check_fitted(solver, who)
    fr = fold_frame.resolve(solver, who, by, fs_dict, b, w)
    K = fr.K
    if isinstance(max_terms, bool) or int(max_terms) != max_terms or not 1 <= int(max_terms) <= K:
        raise ValueError(f"omp_path: max_terms = {max_terms} (1 ... K = {K})")
    S = int(max_terms)
    levels = check_levels(levels, S)
    forced = check_forced(forced, K)
    fold_of_unit, F = fold_frame.deal_units(fr.pt, fr.labels, fr.train, folds, seed)
    method = choose_method(method, K, S)
    Q = levels.size
    table, nsub = fold_frame.plan_table(who, table, F, Q, fr.nclass, K)
    fold_frame.statistics(fr, fold_of_unit, F, nsub)
    if method == "device":
        order, path, held, coef = fr.ctx.omp_path(fr.dptr, K, F, nsub, criterion, forced, S, levels)
    else:
        blocks = download_blocks(fr.ctx, fr.dptr, fr.ncat, K)
        order, path, held, coef = omp_path_host(blocks, K, criterion, forced, S, levels, nsub)
    terms = np.arange(1, S + 1)
    cv_error, cv_se, best, sparsest = cv_picks(terms, held)
    if table == "rows":
        pooled = fold_frame.rows_pooled(fr, coef[:F], F, Q)
        frame = keyed_by_terms(ridge_path.path_table(levels.astype(np.float64), pooled, fr.names))
    else:
        frame = stats_table(levels, held)
    best_terms = None if best is None else int(terms[best])
    return OmpPath(terms, order[F].copy(), order[:F].copy(), levels, coef[F].copy(), path[F, :, 0].copy(), frame, fold_of_unit,
                   cv_error, cv_se, best, best_terms, sparsest, None if sparsest is None else int(terms[sparsest]),
                   selection_frequency(order[:F], best_terms, K))
