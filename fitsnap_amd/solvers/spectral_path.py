"""Grouped K-fold spectral paths: which ridge penalty ``alpha`` and which singular-value cut ``rcond`` predict held-out units
best -- the one knob of ``RIDGE`` and the one knob of ``SVD`` -- from ONE symmetric eigendecomposition per fold.

With the units dealt into F folds and one packed block [G | c | bb, sum wb, n] per (fold, row class) -- ONE pass over the rows,
the layout and statistics of the fold frame --, problem f is "total minus fold f" (f = F: all training rows):

    Qm = T.G - G_f,  qv = T.c - c_f,  y2 = T.bb - bb_f
    dead_j: T.G_jj == 0 or Qm_jj <= loco.PIVOT_TOL T.G_jj  -> no part in the decomposition, coefficient 0;  L: the live columns
    Qm[L, L] = V diag(lambda) V^T  (Jacobi on the unscaled matrix),  z = V^T qv[L],  lambda_max = max |lambda_i|

and every setting q = (alpha >= 0, rcond >= 0) of the product grid is a filter at O(K^2):

    cut = max(rcond^2, 4 n_live eps) lambda_max;   g_i = z_i / (lambda_i + alpha) where lambda_i > cut, else 0;   beta[L] = V g
    rank = #kept,  dof = sum_kept lambda_i / (lambda_i + alpha),  sse = max(y2 - 2 g . z + sum lambda_i g_i^2, 0)

``rcond`` is gelsd's: a cut on the singular values of the weighted rows, so on sqrt(lambda) -- hence rcond^2 -- and ``alpha`` is
``RIDGE``'s, both in unscaled coordinates.  The held-out record of fold f is kept per row class s: (n_{f,s}, bb_{f,s} - 2 beta .
c_{f,s} + beta^T G_{f,s} beta, bb_{f,s}), so the statistics table is split by ``Row_Type`` without a pass over the rows.

The GPU pass is ``fsnap_spectral_path`` (csrc/fsnap_spectral.hip, K <= 144: kernel E1, a batched Jacobi eigensolver with one
workgroup per problem, and kernel E2, the path evaluator); this module holds the same scheme on the host
(``spectral_path_host``: ``_capi.spectral_gram`` over the same downdated systems -- the route of wider systems, the baseline and
the check of the kernel; no GPU needed once the statistics are given), the picks and the tables.  Host and kernel run one text
(csrc/fsnap_spectral_body.h); only the held-out sums, numpy's on the host, are taken in another order.  Fold dealing, block sums,
downdates and the row table are the fold frame's (``folds``; DESIGN.md, "The fold frame").
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from . import folds as fold_frame, ridge_path
from .. import _capi
from .folds import TABLES, download_blocks, sum_blocks, unpack

MAX_K = _capi.SPEC_MAX_K             # fsnap::SPEC_MAX_K
METHODS = ("auto", "device", "host")
PATH_SOLVERS = ("RIDGE", "SVD")
NINFO = 6                            # n_live, sweeps, final off / diag ratio, lambda_max, smallest lambda, status

SpectralPath = namedtuple("SpectralPath", ["alphas", "rconds", "grid", "fits", "rank", "dof", "train_sse", "gcv", "eigenvalues",
                                           "sweeps", "status", "table", "fold_of_unit", "cv_error", "cv_se", "best", "best_alpha",
                                           "best_rcond", "simplest", "simplest_alpha", "simplest_rcond"])


def check_solver(solver):
    """The solver's name; ValueError unless it is a RIDGE or an SVD that does not fit through ``apply_transpose``."""
    kind = type(solver).__name__
    sec = solver.config.sections
    if kind not in PATH_SOLVERS:
        raise ValueError(f"spectral_path: {kind} has no spectral path (only {', '.join(PATH_SOLVERS)} have)")
    if "EXTRAS" in sec and sec["EXTRAS"].apply_transpose:
        raise ValueError("spectral_path: a fit through apply_transpose is a smoother of (G, c), not of the rows")
    return kind


def check_axis(values, name):
    """A grid axis as a float64 vector; ValueError when it is empty or holds a negative or non-finite value."""
    v = np.atleast_1d(np.asarray(values, dtype=np.float64)).reshape(-1)
    if v.size == 0:
        raise ValueError(f"spectral_path: {name} is empty")
    if not np.all(np.isfinite(v)) or np.any(v < 0.0):
        raise ValueError(f"spectral_path: {name} must be finite and >= 0")
    return np.ascontiguousarray(v)


def default_axes(solver, kind, alphas, rconds):
    """(alphas, rconds) with the solver's own setting where an axis is None: RIDGE (its alpha,) x (0,); SVD (0,) x (RCOND,)."""
    if alphas is None:
        alphas = (float(solver.config.sections["RIDGE"].alpha),) if kind == "RIDGE" else (0.0,)
    if rconds is None:
        rconds = (0.0,) if kind == "RIDGE" else (float(type(solver).RCOND),)
    return check_axis(alphas, "alphas"), check_axis(rconds, "rconds")


def choose_method(method, K):
    """"device" (the kernels) or "host".  "auto" takes the kernels wherever they exist (K <= 144) and the host route beyond:
    with Q = 256 the call measured 6.45 ms against 16.71 ms for the host route at 10^6 x 128, F = 5 (6.64 against 80.53 ms at
    F = 40), 0.64 against 2.22 ms on the Ta rows and 10.54 against 20.82 ms at 13 035 x 142 (profiles/spectral_path_timing.txt,
    written by scripts/spectral_path_timing.py)."""
    if method not in METHODS:
        raise ValueError(f"spectral_path: method must be one of {', '.join(METHODS)}")
    if method == "device" and K > MAX_K:
        raise ValueError(f"spectral_path: method='device' needs K <= {MAX_K} (K = {K})")
    if method == "auto":
        return "device" if K <= MAX_K else "host"
    return method


def spectral_path_host(blocks, K, alphas, rconds, nsub=1, threads=None):
    """``fsnap_spectral_path`` on the host from the downloaded ``blocks`` (F * nsub rows of K^2 + K + 3 doubles): the same sums,
    downdates and dead-column rule, ``_capi.spectral_gram`` per problem from a pool of ``threads`` Python threads (default: at
    most 16; the library call releases the interpreter lock).  Any K.  Returns what ``HipContext.spectral_path`` returns:
    (eig, z, info, sets, fits, coef, heldout)."""
    alphas, rconds = check_axis(alphas, "alphas"), check_axis(rconds, "rconds")
    blocks = np.asarray(blocks, dtype=np.float64)
    folds, total = sum_blocks(blocks, nsub)
    F, Q = folds.shape[0], alphas.size * rconds.size
    eig, z, info = np.zeros((F + 1, K)), np.zeros((F + 1, K)), np.zeros((F + 1, NINFO))
    sets = np.zeros((F + 1, Q, 3))
    coef = np.zeros((F + 1, Q, K))
    held = np.zeros((F, Q, nsub, 3))
    tdiag = np.ascontiguousarray(np.diag(unpack(total, K)[0]))

    def solve(f):
        Qm, qv, y2, _, _ = fold_frame.downdated(folds, total, f, K)
        r = _capi.spectral_gram(Qm, qv, y2, alphas, rconds, tdiag)
        eig[f], z[f] = r.eig, r.z
        info[f] = (r.n_live, r.sweeps, r.off_ratio, r.lambda_max, r.lambda_min, r.status)
        sets[f, :, 0], sets[f, :, 1], sets[f, :, 2] = r.rank.reshape(-1), r.dof.reshape(-1), r.sse.reshape(-1)
        beta = r.coef.reshape(Q, K)
        coef[f] = beta
        if f < F:
            for s in range(nsub):
                G, c, bb, n = unpack(blocks[f * nsub + s], K)
                held[f, :, s, 0] = n
                held[f, :, s, 1] = bb - 2.0 * (beta @ c) + np.einsum("qi,qi->q", beta @ G, beta)
                held[f, :, s, 2] = bb

    fold_frame.run_pool(solve, F + 1, threads)
    return eig, z, info, sets, coef[F].copy(), coef[:F].copy(), held


def class_sum(heldout):
    """(F x Q x 3) records of the folds from the (F x Q x nsub x 3) per-class records, the classes added in index order."""
    heldout = np.asarray(heldout, dtype=np.float64)
    out = heldout[:, :, 0, :].copy()
    for s in range(1, heldout.shape[2]):
        out = out + heldout[:, :, s, :]
    return out


def picks(alphas, rconds, cv_error, cv_se, dof):
    """(best, simplest) among the Q = Qa Qr settings q = ia Qr + ir.  best: the smallest finite ``cv_error``; ties go to the
    larger alpha, then to the larger rcond.  simplest: the smallest ``dof`` (of the fit on all rows) among the settings with
    cv_error <= cv_error[best] + cv_se[best]; ties go to the smaller cv_error, then as for best.  Both None when no setting has
    a finite error."""
    alphas, rconds = np.asarray(alphas, dtype=np.float64), np.asarray(rconds, dtype=np.float64)
    Qr = rconds.size
    Q = alphas.size * Qr

    def stronger(q, r):                                     # q regularises more than r
        a, b = (alphas[q // Qr], rconds[q % Qr]), (alphas[r // Qr], rconds[r % Qr])
        return a > b

    best = None
    for q in range(Q):
        if not np.isfinite(cv_error[q]):
            continue
        if best is None or cv_error[q] < cv_error[best] or (cv_error[q] == cv_error[best] and stronger(q, best)):
            best = q
    if best is None:
        return None, None
    bar = cv_error[best] + (cv_se[best] if np.isfinite(cv_se[best]) else 0.0)
    simplest = best
    for q in range(Q):
        if not (np.isfinite(cv_error[q]) and cv_error[q] <= bar):
            continue
        s = simplest
        if dof[q] < dof[s] or (dof[q] == dof[s] and (cv_error[q] < cv_error[s] or (cv_error[q] == cv_error[s] and stronger(q, s)))):
            simplest = q
    return best, simplest


def grid_index(alphas, rconds):
    """The (alpha, rcond) of every setting q = ia Qr + ir, as a list of tuples of floats."""
    return [(float(a), float(r)) for a in alphas for r in rconds]


def stats_table(alphas, rconds, heldout, names=None):
    """``table="stats"``: DataFrame indexed (alpha, rcond, Row_Type) with an ``*ALL`` row and, where the records are per row
    class (``names``: one per class), one row per row type; ncount and w_rmse from the statistics form of the held-out error
    (F x Q x nsub x 3), mae and rmse (which need the rows) NaN."""
    from pandas import DataFrame, MultiIndex

    heldout = np.asarray(heldout, dtype=np.float64)
    nsub = heldout.shape[2]
    per = np.zeros(heldout.shape[1:])                       # Q x nsub x 3, the folds added in index order
    for f in range(heldout.shape[0]):
        per = per + heldout[f]
    index, rows = [], []

    def metrics(n, sse):
        return (int(n), np.nan, np.nan, np.sqrt(max(sse, 0.0) / n) if n > 0 else np.nan)

    for q, (a, r) in enumerate(grid_index(alphas, rconds)):
        index.append((a, r, "*ALL"))
        rows.append(metrics(per[q, :, 0].sum(), per[q, :, 1].sum()))
        if names is not None and nsub == len(names):
            for s, name in enumerate(names):
                index.append((a, r, name))
                rows.append(metrics(per[q, s, 0], per[q, s, 1]))
    return DataFrame(rows, index=MultiIndex.from_tuples(index, names=["alpha", "rcond", "Row_Type"]),
                     columns=["ncount", "mae", "rmse", "w_rmse"])


def rows_table(alphas, rconds, pooled, names):
    """``table="rows"``: ``ridge_path.path_table`` of the pooled row sums (Q x nclass x 4), re-keyed (alpha, rcond, Row_Type)."""
    from pandas import MultiIndex

    grid = grid_index(alphas, rconds)
    frame = ridge_path.path_table(np.arange(len(grid), dtype=np.float64), pooled, names)
    frame.index = MultiIndex.from_tuples([grid[int(q)] + (name,) for q, name in frame.index], names=["alpha", "rcond", "Row_Type"])
    return frame


def spectral_path(solver, alphas=None, rconds=None, folds=5, by="Configs", fs_dict=None, b=None, w=None, method="auto",
                  table="auto", seed=0):
    """``Solver.spectral_path``: see there."""
    who = "spectral_path"
    kind = check_solver(solver)                             # every rank refuses alike
    alphas, rconds = default_axes(solver, kind, alphas, rconds)
    if method not in METHODS:
        raise ValueError(f"spectral_path: method must be one of {', '.join(METHODS)}")
    if table not in TABLES:
        raise ValueError(f"spectral_path: table must be one of {', '.join(TABLES)}")
    fold_frame.check_fitted(solver, who)
    fr = fold_frame.resolve(solver, who, by, fs_dict, b, w)
    K, Qr = fr.K, rconds.size
    Q = alphas.size * Qr
    method = choose_method(method, K)
    fold_of_unit, F = fold_frame.deal_units(fr.pt, fr.labels, fr.train, folds, seed)
    table, nsub = fold_frame.plan_table(who, table, F, Q, fr.nclass, K)
    fold_frame.statistics(fr, fold_of_unit, F, nsub)
    if method == "device":
        eig, _, info, sets, fits, coef, held = fr.ctx.spectral_path(fr.dptr, K, F, nsub, alphas, rconds, table == "rows")
    else:
        blocks = download_blocks(fr.ctx, fr.dptr, fr.ncat, K)
        eig, _, info, sets, fits, coef, held = spectral_path_host(blocks, K, alphas, rconds, nsub)
    folded = class_sum(held)
    cv_error, cv_se, _, _ = fold_frame.cv_curve(np.zeros(Q), folded)
    dof, sse = sets[F, :, 1].copy(), sets[F, :, 2].copy()
    n = float(folded[:, 0, 0].sum())
    with np.errstate(divide="ignore", invalid="ignore"):
        gcv = n * sse / (n - dof) ** 2
    best, simplest = picks(alphas, rconds, cv_error, cv_se, dof)
    if table == "rows":
        frame = rows_table(alphas, rconds, fold_frame.rows_pooled(fr, coef, F, Q), fr.names)
    else:
        frame = stats_table(alphas, rconds, held, fr.names)
    grid = grid_index(alphas, rconds)

    def axis(q, values, which):
        return None if q is None else float(values[q // Qr if which == 0 else q % Qr])

    return SpectralPath(alphas, rconds, grid, fits, sets[:, :, 0].astype(np.int64), sets[:, :, 1].copy(), sets[:, :, 2].copy(), gcv,
                        eig, info[:, 1].astype(np.int64), info[:, 5].astype(np.int64), frame, fold_of_unit, cv_error, cv_se, best,
                        axis(best, alphas, 0), axis(best, rconds, 1), simplest, axis(simplest, alphas, 0),
                        axis(simplest, rconds, 1))
