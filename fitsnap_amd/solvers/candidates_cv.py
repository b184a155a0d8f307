"""Grouped K-fold cross-validation of the weight candidates of ``CandidateFits`` (``CandidateFits.cross_validate``).

The weight search scores a candidate by its errors on the rows it was fitted to.  Here the units (configurations) are dealt into
F folds (``folds.deal_folds``), every candidate is refitted F times with one fold left out, and every row is scored under
the refit that did not see its unit.  With one packed block of statistics per (fold, category) -- ONE pass over the rows,
``fsnap_cat_prepare`` + ``fsnap_cat_normal_eq`` with the composite category fold * C + c -- the refit (p, f) is

    Qm = sum_c S[p, c]^2 (T[c].G - B[f, c].G),   qv = sum_c S[p, c]^2 (T[c].r - B[f, c].r),   T[c] = sum_f B[f, c]

solved on the GPU by ``fsnap_cv_candidates`` (csrc/fsnap_cv.hip, K <= 144) and scored by ``fsnap_cv_candidate_rows``, which
reads every row once per 16 candidates.  This module holds the routes, the pooling of the held-out sums and the tables.
"""
from __future__ import annotations

import numpy as np

from .. import _capi
from . import folds as fold_frame

MAX_K = 144                  # fsnap::CV_MAX_K
METHODS = ("auto", "device", "composed")
METRICS = {"mae": 0, "rmse": 1}
COLUMNS = ["ncount", "mae", "rmse", "w_mae", "w_rmse"]


def choose_method(method, K):
    """"device", "auto" or "composed" for K columns; ValueError for an unknown method or method="device" beyond K = 144.
    "auto" beyond 144 columns is the composed route."""
    if method not in METHODS:
        raise ValueError(f"cross_validate: method must be one of {', '.join(METHODS)}")
    if method == "device" and K > MAX_K:
        raise ValueError(f"cross_validate: method='device' needs K <= {MAX_K} (K = {K})")
    if method == "auto" and K > MAX_K:
        return "composed"
    return method


def composite_scales(S, F, problems=None):
    """The scale matrix of the composed route: row (p, f) scales composite category (f', c) by S[p, c] [f' != f] -- exactly
    zero on the held-out fold.  (P F, F C) for all problems, or one row per (p, f) pair of ``problems``."""
    S = np.asarray(S, dtype=np.float64)
    P, C = S.shape
    if problems is None:
        problems = [(p, f) for p in range(P) for f in range(F)]
    out = np.empty((len(problems), F * C))
    for i, (p, f) in enumerate(problems):
        out[i] = np.tile(S[p], F)
        out[i, f * C:(f + 1) * C] = 0.0
    return out


def own_fold(sums_pf, P, F, C):
    """(P, F C, 4) from the sums of P F vectors over all F C composite categories (``fsnap_candidate_rows``): of vector
    (p, f) only the categories of its own fold f are kept."""
    sums_pf = np.asarray(sums_pf, dtype=np.float64).reshape(P, F, F, C, 4)
    out = np.empty((P, F, C, 4))
    for f in range(F):
        out[:, f] = sums_pf[:, f, f]
    return out.reshape(P, F * C, 4)


def pool_heldout(sums4, counts, S, F):
    """(P, C, 5) pooled n, sum|r|, sum r^2, sum|w r|, sum (w r)^2 of the held-out rows with the candidate's weights
    w = w0 S[p, c], from sums4 (P, F C, 4: sum|r|, sum r^2, sum|w0 r|, sum (w0 r)^2 per composite category) and counts (F C rows
    per composite category).  Folds are added in index order."""
    S = np.asarray(S, dtype=np.float64)
    P, C = S.shape
    sums4 = np.asarray(sums4, dtype=np.float64).reshape(P, F, C, 4)
    counts = np.asarray(counts, dtype=np.float64).reshape(F, C)
    pooled = np.zeros((P, C, 5))
    for f in range(F):
        pooled[:, :, 0] += counts[f][None, :]
        pooled[:, :, 1:] += sums4[:, f]
    pooled[:, :, 3] *= np.abs(S)
    pooled[:, :, 4] *= S * S
    return pooled


def metrics(sums):
    """(..., 5) ncount, mae, rmse, w_mae, w_rmse from (..., 5) pooled sums; NaN where there is no row."""
    sums = np.asarray(sums, dtype=np.float64)
    n = sums[..., 0]
    with np.errstate(divide="ignore", invalid="ignore"):
        out = np.stack([n, sums[..., 1] / n, np.sqrt(sums[..., 2] / n), sums[..., 3] / n, np.sqrt(sums[..., 4] / n)], axis=-1)
    out[..., 1:][n == 0] = np.nan
    return out


class CandidateCV:
    """Result of ``CandidateFits.cross_validate``.

    ``coef`` (P, F, K): the refit of candidate p without fold f; ``status`` (P, F): 0, or 1 where the refit failed (NaN
    coefficients); ``min_pivot`` (P, F): smallest pivot of the Jacobi-scaled matrix (NaN where the composed route solved);
    ``route`` (P, F) of "device" / "composed"; ``fold_of_unit``: {unit: fold}; ``sums`` (P, C, 5): per candidate and category
    of ``keys`` the pooled n, sum|r|, sum r^2, sum|w r|, sum (w r)^2 of the held-out rows, w = w0 S[p, c] (testing categories
    hold no row); ``row_types``: the row types in sorted order; ``base_sums`` (P, C, 5): the same sums with the base weights
    w0 alone (no scaling by S), the sums the objective of ``cross_validate_gradient`` is taken on (None when not given)."""

    def __init__(self, coef, status, min_pivot, route, fold_of_unit, sums, keys, S, base_sums=None):
        self.coef = coef
        self.status = status
        self.min_pivot = min_pivot
        self.route = route
        self.fold_of_unit = fold_of_unit
        self.sums = sums
        self.keys = list(keys)
        self.S = S
        self.base_sums = base_sums
        self.row_types = sorted({k[2] for k in self.keys})

    def _groups(self):
        """([(group, row type)] of the training categories, their positions in keys)."""
        at = [i for i, k in enumerate(self.keys) if not k[1]]
        return [(self.keys[i][0], self.keys[i][2]) for i in at], at

    def _type_sums(self):
        """(P, ntypes, 5): the sums pooled over all groups per row type, categories added in ``keys`` order."""
        out = np.zeros((self.sums.shape[0], len(self.row_types), 5))
        for i, k in enumerate(self.keys):
            if not k[1]:
                out[:, self.row_types.index(k[2])] += self.sums[:, i]
        return out

    def tables(self, frames=True):
        """Per candidate the held-out error table: a DataFrame indexed (Groups, Row_Type), the training categories in ``keys``
        order and one ``*ALL`` row per row type after them, columns ncount, mae, rmse, w_mae, w_rmse (the weighted columns
        over all ncount rows).  ``frames=False``: (index list, array (P, rows, 5))."""
        index, at = self._groups()
        values = np.concatenate([metrics(self.sums[:, at]), metrics(self._type_sums())], axis=1)
        index = index + [("*ALL", t) for t in self.row_types]
        if not frames:
            return index, values
        from pandas import DataFrame, MultiIndex

        mi = MultiIndex.from_tuples(index, names=["Groups", "Row_Type"])
        return [DataFrame(values[p], index=mi, columns=COLUMNS) for p in range(values.shape[0])]

    @property
    def row_type_errors(self):
        """(P, ntypes, 2): mae and rmse over all held-out rows of a row type (``row_types`` order)."""
        return metrics(self._type_sums())[:, :, 1:3]

    def cost(self, weights, metric="rmse"):
        """(P,) sum_t weights[t] * metric_t over the row types: the objective of the weight search (``fit_and_cost``:
        etot_weight * rmse_E + ftot_weight * rmse_F + stress_weight * rmse_S) on held-out rows.  ``weights``: a mapping from
        row type to weight (missing types count 0) or one weight per entry of ``row_types``.  A row type of weight 0 takes no
        part; a candidate with any failed fold has NaN cost."""
        if metric not in METRICS:
            raise ValueError(f"cost: metric must be one of {', '.join(METRICS)}")
        if hasattr(weights, "keys"):
            unknown = [t for t in weights if t not in self.row_types]
            if unknown:
                raise ValueError(f"cost: no rows of type {unknown[0]!r} (row types: {self.row_types})")
            wt = np.array([float(weights.get(t, 0.0)) for t in self.row_types])
        else:
            wt = np.asarray(weights, dtype=np.float64).reshape(-1)
            if wt.shape[0] != len(self.row_types):
                raise ValueError(f"cost: {wt.shape[0]} weights for the row types {self.row_types}")
        err = self.row_type_errors[:, :, METRICS[metric]]
        out = np.zeros(err.shape[0])
        for t in range(len(self.row_types)):
            if wt[t] != 0.0:
                out = out + wt[t] * err[:, t]
        out[np.asarray(self.status).any(axis=1)] = np.nan
        return out


def fold_key(folds, by, seed):
    """A hashable description of the fold assignment asked for: equal keys give equal folds on the same labels."""
    if folds is None:
        return ("units", by)
    if hasattr(folds, "keys"):
        return ("mapping", by, tuple(sorted((str(k), str(folds[k])) for k in folds)))
    return ("dealt", by, folds, seed)


def composite_layout(cf, folds, by, seed):
    """(composite categories per row, fold_of_unit, F) of the CandidateFits ``cf``: units from ``fs_dict[by]`` over the
    training rows, folds from ``folds.deal_units`` (collective: a unit gets one fold on every rank)."""
    if by not in cf.fs_dict:
        raise KeyError(f"cross_validate: fs_dict has no {by!r} labels to take the units from")
    labels = cf.fs_dict[by]
    if len(labels) != cf.m:
        raise ValueError(f"cross_validate: fs_dict[{by!r}] must have one entry per row")
    train = ~cf.testing
    fold_of_unit, F = fold_frame.deal_units(cf.pt, labels, train, folds, seed)
    if F < 2:
        raise ValueError(f"cross_validate: {F} fold; at least 2 are needed to hold rows out")
    K, C = cf.K, cf.ncat
    if F * C * (K * K + K + 3) * 8 > fold_frame.CAT_STATS_MAX_BYTES:
        raise ValueError(f"cross_validate: {F} folds x {C} categories of statistics of order {K} exceed "
                         "FSNAP_CAT_STATS_MAX_BYTES; use fewer folds")
    fold = fold_frame.row_categories(labels, train, fold_of_unit, None, 1)
    ccat = np.where((fold >= 0) & (cf.cat >= 0), fold * C + cf.cat, -1).astype(np.int32)
    return ccat, fold_of_unit, F


def cross_validate(cf, S, folds=5, by="Configs", seed=0, method="auto"):
    """``CandidateFits.cross_validate``: see there."""
    from .candidates import check_scales

    S = check_scales(S, cf.ncat)
    P, C, K = S.shape[0], cf.ncat, cf.K
    method = choose_method(method, K)
    # the labels are walked once per (folds, by, seed): a search calls this once per generation with the same folds
    key = fold_key(folds, by, seed)
    if cf._cv_folds is None or cf._cv_folds[0] != key:
        ccat, fold_of_unit, F = composite_layout(cf, folds, by, seed)
        cf._cv_folds = (key, ccat, fold_of_unit, F, np.bincount(ccat[ccat >= 0], minlength=F * cf.ncat))
    _, ccat, fold_of_unit, F, counts = cf._cv_folds
    kind, param, _ = cf._kind()
    alpha = float(param) if kind in (_capi.SOLVE_RIDGE, _capi.SOLVE_RIDGE_INV) else 0.0
    ctx = cf._cv_device(ccat, F)
    tag = cf._cv[0]
    coef = np.full((P, F, K), np.nan)
    status = np.zeros((P, F), dtype=np.int64)
    min_pivot = np.full((P, F), np.nan)
    route = np.full((P, F), "device", dtype=object)
    todo = []
    if method in ("device", "auto"):
        coef, info = ctx.cv_candidates(tag, alpha, S, F, K)
        status = info[:, :, 0].astype(np.int64)
        min_pivot = info[:, :, 1].copy()
        if method == "auto":
            todo = [(int(p), int(f)) for p, f in zip(*np.nonzero(status))]
    else:
        todo = [(p, f) for p in range(P) for f in range(F)]
    if todo:
        betas = composed_fits(cf, ctx, tag, kind, param, composite_scales(S, F, todo))
        for (p, f), beta in zip(todo, betas):
            coef[p, f] = beta
            route[p, f] = "composed"
            status[p, f] = 0 if np.isfinite(beta).all() else 1
    if cf.m > 0:
        if method == "composed":
            full = ctx.candidate_rows(tag, coef.reshape(P * F, K), None, _capi.CAND_ERROR_SUMS, F * C)
            sums4 = own_fold(full, P, F, C)
        else:
            sums4 = ctx.cv_candidate_rows(tag, coef, C)
        pooled = pool_heldout(sums4, counts, S, F)
        base = pool_heldout(sums4, counts, np.ones_like(S), F)
    else:
        pooled = np.zeros((P, C, 5))
        base = np.zeros((P, C, 5))
    if cf.pt.multi:
        both = np.ascontiguousarray(np.stack([pooled, base]))        # one elementwise all-reduce for the two
        cf.pt.allreduce_host(both.reshape(-1))
        pooled, base = both[0], both[1]
    return CandidateCV(coef, status, min_pivot, route, dict(fold_of_unit), pooled, cf.keys, S, base)


def composed_fits(cf, ctx, tag, kind, param, Sc):
    """The route that exists without the kernels of csrc/fsnap_cv.hip: ``fsnap_fit_candidates`` on the composite layout with
    the scale rows ``Sc`` (zero on the held-out fold), followed by the solver's own truncating solve where the probe says so
    -- as ``fit`` does, but with no refinement and no row-space solve."""
    K = cf.K
    T = K * K + K + 3
    betas, ranks, _, dptr = ctx.fit_candidates(tag, _capi.PROBE_OF[kind], param, Sc, K)
    for i in range(Sc.shape[0]):
        if int(ranks[i]) < 0:
            G, c, _ = ctx.download_packed(dptr + i * T * 8, K)
            betas[i] = cf.solver._solve(kind, param, G, c)
    return betas
