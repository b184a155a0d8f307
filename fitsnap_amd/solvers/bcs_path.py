"""Grouped K-fold BCS sparsity paths: which ``[BCS]`` setting (``sigma2`` or ``scale``, ``eta``, ``itermax``) predicts held-out
units best, how many descriptors it keeps, and the posterior covariance that comes with it.

The initial noise variance sets the sparsity of a BCS fit and the iteration cap how far the recurrence gets; the reference
fixes both (``scale`` = 0.01, 10 iterations), which is why its documentation says the solver does not prune properly yet.
Every iteration of ``bcs()`` touches the weighted training rows only through (A^T A, A^T y, |y|^2, sum y, n).  With the units
dealt into F folds and one packed block [G_f | c_f | bb_f, sum wb_f, n_f] per fold -- ONE pass over the rows, the layout and
statistics of the fold frame --, problem (f, q) is the BCS fit of setting q on "total minus block f" (f = F: on all training
rows):

    Qm = T.G - G_f,  qv = T.c - c_f,  y2 = T.bb - bb_f,  sum_y = T.sum wb - sum wb_f,  n = T.n - n_f
    dead_j: T.G_jj == 0 or Qm_jj <= loco.PIVOT_TOL T.G_jj  -> never a candidate, coefficient 0
    sigma2 = the setting's, or max(scale (y2 / n - (sum_y / n)^2), 1e-16) from the problem's OWN scalars

followed by ``fsnap_bcs_gram``'s recurrence (include/fsnap_hip.h) with the ``[BCS]`` ``max_active`` and ``deletion``.

The GPU pass is ``fsnap_bcs_path`` (csrc/fsnap_bcs.hip, K <= 144 and max_active <= 64, one workgroup per problem); this module
holds the grid, the same scheme on the host (``bcs_path_host``: ``_capi.bcs_gram`` over the same downdated systems -- the route
of wider systems, the baseline and the check of the kernel; no GPU needed once the statistics are given) and the picks.  The
two routes run one text, sum for sum; only the device's ``log`` (in principle) and the order of the held-out sums are not the
host's, so the fits agreed to the bit on every case measured and the held-out errors to the rounding of their cancelling
terms.  The picks of the two routes are compared where ``margin`` (the smallest relative gap between the best and the
second-best marginal likelihood of an iteration) is well above rounding.  Fold dealing, block sums, downdates and tables are the fold frame's
(``folds``; DESIGN.md, "The fold frame").
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from . import folds as fold_frame, ridge_path
from .. import _capi
from .ard_path import cv_picks, setting_index
from .folds import TABLES, download_blocks, stats_table, sum_blocks, unpack

MAX_K = _capi.BCS_MAX_K              # fsnap::BCS_MAX_K
MAX_ACTIVE = _capi.BCS_MAX_ACTIVE    # fsnap::BCS_MAX_ACTIVE
MAX_ITER = 65536                     # the largest itermax fsnap_bcs_path takes
METHODS = ("auto", "device", "host")
KEYS = ("scale", "sigma2", "eta", "itermax")
NHYPER = 4                           # sigma2 or 0, scale, eta, itermax
NINFO = 6                            # iterations, status, sigma2 used, sigma2 re-estimated, rss, margin

BcsPath = namedtuple("BcsPath", ["grid", "fits", "nonzeros", "active", "errbars", "covs", "sigma2", "iterations", "status",
                                 "margin", "picks", "table", "fold_of_unit", "cv_error", "cv_se", "best", "best_setting",
                                 "sparsest", "sparsest_setting", "frequency"])


def check_solver(solver):
    """ValueError unless the solver is a BCS that does not fit through ``apply_transpose``."""
    kind = type(solver).__name__
    sec = solver.config.sections
    if kind != "BCS":
        raise ValueError(f"bcs_path: {kind} has no BCS path (only BCS has; LASSO has lasso_path, ARD ard_path, OMP omp_path)")
    if "EXTRAS" in sec and sec["EXTRAS"].apply_transpose:
        raise ValueError("bcs_path: a fit through apply_transpose has no rows to hold out (its samples are the columns of G)")


def resolve_max_active(max_active, K):
    """``[BCS] max_active`` for K columns: 0 stands for min(K, 64), what the kernel holds; ValueError beyond K."""
    if max_active > K:
        raise ValueError(f"BCS: max_active = {max_active} for {K} columns")
    return int(max_active) if max_active > 0 else min(K, MAX_ACTIVE)


def choose_method(method, K, max_active=None):
    """"device" (the kernel) or "host".  "auto" takes the kernel wherever it exists (K <= 144, max_active <= 64) and the host
    route beyond: at F = 5, Q = 8 (48 problems, itermax = 80) the kernel call measured 0.89 ms against 8.90 ms for the host
    route at 10^6 x 128 (10.0 x) and 0.63 ms against 6.47 ms on the Ta rows (profiles/bcs_path_timing.txt, written by
    scripts/bcs_path_timing.py).  The kernel is the faster route already at 48 problems, so there is no break-even number of
    problems below which "auto" would go to the host."""
    if method not in METHODS:
        raise ValueError(f"bcs_path: method must be one of {', '.join(METHODS)}")
    fits = K <= MAX_K and (max_active is None or max_active <= MAX_ACTIVE)
    if method == "device" and not fits:
        raise ValueError(f"bcs_path: method='device' needs K <= {MAX_K} and max_active <= {MAX_ACTIVE} (K = {K}, max_active = "
                         f"{max_active})")
    if method == "auto":
        return "device" if fits else "host"
    return method


def resolve_grid(grid, section):
    """The grid as a list of complete mappings.  Every entry overrides keys of the ``[BCS]`` section: ``sigma2`` (None: from
    ``scale``), ``scale``, ``eta``, ``itermax``; a bare number stands for ``scale``.  ValueError for an empty grid, an unknown
    key, a value that is not finite, ``sigma2`` or ``scale`` <= 0, ``eta`` < 0 or an ``itermax`` outside 1 ... 65 536."""
    if hasattr(grid, "keys") or isinstance(grid, (str, bytes)) or not hasattr(grid, "__iter__"):
        raise ValueError("bcs_path: the grid must be a sequence of mappings or of numbers")
    out = []
    for entry in grid:
        if not hasattr(entry, "keys"):
            entry = {"scale": entry}
        unknown = [k for k in entry if k not in KEYS]
        if unknown:
            raise ValueError(f"bcs_path: unknown grid key {unknown[0]!r} ({', '.join(KEYS)})")
        full = {k: entry[k] if k in entry else getattr(section, k) for k in KEYS}
        full["sigma2"] = None if full["sigma2"] is None else float(full["sigma2"])
        full["scale"], full["eta"] = float(full["scale"]), float(full["eta"])
        it = full["itermax"]
        if isinstance(it, bool) or int(it) != it or not 1 <= int(it) <= MAX_ITER:
            raise ValueError(f"bcs_path: grid value itermax = {it} (1 ... {MAX_ITER})")
        full["itermax"] = int(it)
        s2, sc, eta = full["sigma2"], full["scale"], full["eta"]
        if s2 is not None and not (np.isfinite(s2) and s2 > 0.0):
            raise ValueError(f"bcs_path: grid value sigma2 = {s2}")
        if not (np.isfinite(sc) and sc > 0.0):
            raise ValueError(f"bcs_path: grid value scale = {sc}")
        if not (np.isfinite(eta) and eta >= 0.0):
            raise ValueError(f"bcs_path: grid value eta = {eta}")
        out.append(full)
    if not out:
        raise ValueError("bcs_path: the grid is empty")
    return out


def hyper_of(grid):
    """(Q x 4) rows (sigma2 or 0, scale, eta, itermax) of the complete settings ``grid``, as ``fsnap_bcs_path`` takes them."""
    return np.array([[0.0 if g["sigma2"] is None else g["sigma2"], g["scale"], g["eta"], float(g["itermax"])] for g in grid],
                    dtype=np.float64).reshape(len(grid), NHYPER)


def bcs_path_host(blocks, K, hyper, max_active, deletion="reference", nsub=1, threads=None):
    """``fsnap_bcs_path`` on the host from the downloaded ``blocks`` (F * nsub rows of K^2 + K + 3 doubles): the same sums,
    downdates and dead-column rule, ``_capi.bcs_gram`` per problem from a pool of ``threads`` Python threads (default: at most
    16; the library call releases the interpreter lock).  Any K, any max_active <= K.  Returns what ``HipContext.bcs_path``
    returns: (coef, active, alpha, errbars, picks, info, heldout, Sig)."""
    hyper = np.asarray(hyper, dtype=np.float64)
    if hyper.ndim != 2 or hyper.shape[1] != NHYPER:
        raise ValueError(f"bcs_path: hyper has shape {hyper.shape}, not (Q, {NHYPER})")
    folds, total = sum_blocks(blocks, nsub)
    F, Q, MA = folds.shape[0], hyper.shape[0], int(max_active)
    P = int(hyper[:, 3].max())
    coef = np.zeros((F + 1, Q, K))
    active = np.full((F + 1, Q, MA), -1, dtype=np.int32)
    alpha = np.zeros((F + 1, Q, MA))
    err = np.zeros((F + 1, Q, MA))
    picks = np.full((F + 1, Q, P, 2), -1, dtype=np.int32)
    info = np.zeros((F + 1, Q, NINFO))
    held = np.zeros((F, Q, 3))
    Sig = np.zeros((Q, MA, MA))
    tdiag = np.ascontiguousarray(np.diag(unpack(total, K)[0]))
    at = K * K + K
    systems = [fold_frame.downdated(folds, total, f, K) for f in range(F + 1)]

    def solve(p):
        f, q = divmod(p, Q)
        Qm, qv, y2, n, _ = systems[f]
        sum_y = total[at + 1] - folds[f, at + 1] if f < F else total[at + 1]
        s2, scale, eta, itermax = hyper[q]
        r = _capi.bcs_gram(Qm, qv, y2, sum_y, n, s2 if s2 > 0.0 else None, scale, eta, int(itermax), MA, deletion, tdiag)
        na = r.active.size
        coef[f, q] = r.coef
        active[f, q, :na], alpha[f, q, :na], err[f, q, :na] = r.active, r.alpha, r.errbars
        picks[f, q, :int(itermax)] = r.picks
        info[f, q] = (r.iterations, r.status, r.sigma2_in, r.sigma2, r.rss, r.margin)
        if f < F:
            G, c, bb, nf = unpack(folds[f], K)
            held[f, q] = (nf, bb - 2.0 * (r.coef @ c) + r.coef @ (G @ r.coef), bb)
        else:
            Sig[q, :na, :na] = r.Sig

    fold_frame.run_pool(solve, (F + 1) * Q, threads)
    return coef, active, alpha, err, picks, info, held, Sig


def covariances(fits, active, Sig):
    """(Q x K x K) covariances of the fits on all rows as ``BCS.perform_fit`` forms them: diag(fit^2) with the support block
    set to ``Sig``, negative entries clipped to 0."""
    Q, K = fits.shape
    covs = np.zeros((Q, K, K))
    for q in range(Q):
        beta = np.nan_to_num(fits[q])
        covs[q] = np.diag(beta ** 2)
        sup = active[q][active[q] >= 0]
        block = Sig[q, :sup.size, :sup.size]
        covs[q][np.ix_(sup, sup)] = np.where(block < 0.0, 0.0, block)
    return covs


def keep_frequency(fold_active, best, K):
    """Per column, the share of the fold refits at setting ``best`` that kept it (zeros without a pick)."""
    freq = np.zeros(K)
    if best is None or fold_active.shape[0] == 0:
        return freq
    for a in fold_active[:, best]:
        freq[a[a >= 0]] += 1.0
    return freq / fold_active.shape[0]


def bcs_path(solver, grid, folds=5, by="Configs", fs_dict=None, b=None, w=None, method="auto", table="auto", seed=0):
    """``Solver.bcs_path``: see there."""
    who = "bcs_path"
    check_solver(solver)                                    # every rank refuses alike
    section = solver.config.sections["BCS"]
    grid = resolve_grid(grid, section)
    if method not in METHODS:
        raise ValueError(f"bcs_path: method must be one of {', '.join(METHODS)}")
    if table not in TABLES:
        raise ValueError(f"bcs_path: table must be one of {', '.join(TABLES)}")
    fold_frame.check_fitted(solver, who)
    fr = fold_frame.resolve(solver, who, by, fs_dict, b, w)
    K, Q = fr.K, len(grid)
    max_active = resolve_max_active(section.max_active, K)
    method = choose_method(method, K, max_active)
    fold_of_unit, F = fold_frame.deal_units(fr.pt, fr.labels, fr.train, folds, seed)
    table, nsub = fold_frame.plan_table(who, table, F, Q, fr.nclass, K)
    fold_frame.statistics(fr, fold_of_unit, F, nsub)
    hyper = hyper_of(grid)
    if method == "device":
        coef, active, _, err, picks, info, held, Sig = fr.ctx.bcs_path(fr.dptr, K, F, nsub, hyper, max_active, section.deletion)
    else:
        blocks = download_blocks(fr.ctx, fr.dptr, fr.ncat, K)
        coef, active, _, err, picks, info, held, Sig = bcs_path_host(blocks, K, hyper, max_active, section.deletion, nsub)
    status = info[:, :, 1].astype(np.int64)
    held[:F][status[:F] == 1, 1] = np.nan
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
    return BcsPath(grid, fits, nonzeros, active[F].copy(), err[F].copy(), covariances(fits, active[F], Sig), info[:, :, 3].copy(),
                   info[:, :, 0].astype(np.int64), status, info[:, :, 5].copy(), picks, setting_index(frame), fold_of_unit,
                   cv_error, cv_se, best, None if best is None else grid[best], sparsest,
                   None if sparsest is None else grid[sparsest], keep_frequency(active[:F], best, K))
