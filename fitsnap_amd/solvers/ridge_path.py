"""Exact leave-one-unit-out error of ridge fits as a function of alpha (what RidgeCV is to Ridge).

With the weighted training rows x_i = w_i a_i, y_i = w_i b_i of the last fit, G = sum x x^T and c = sum x y, every unit u
(a configuration, or any label such as a group) and every grid point alpha_q >= 0 gets the REFIT without the unit's rows

    G_u = X_u^T X_u,  c_u = X_u^T y_u                          (once per unit, shared by all alphas)
    B_q = G - G_u + alpha_q I,  D_q = sqrt(diag B_q),  H_q = D_q^-1 B_q D_q^-1
    beta_{q,-u} = D_q^-1 H_q^-1 D_q^-1 (c - c_u)               (Cholesky of H_q, pivot check)
    p_i^q = a_i . beta_{q,-u},  r_i^q = b_i - p_i^q            for every row i of u

A unit is not identifiable at alpha_q when a diagonal entry of B_q is <= 0 -- in floating point: has cancelled to at most
``loco.PIVOT_TOL`` (G_jj + alpha_q), the downdate of a column the unit alone touches leaves rounding noise of either sign --
or a pivot of H_q is <= ``loco.PIVOT_TOL``: its rows get NaN there and its sums are zero.  The GPU pass is
``fsnap_ridge_path`` (csrc/fsnap_path.hip, K <= 144); this module holds the same closed form in numpy
(``ridge_path_host``, the check of the kernel), the composed route through ``fsnap_loco_rows``
(``method="woodbury"``: per alpha a factor and a Woodbury pass; the baseline, and the route of wider systems) and the tables.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from . import loco

MAX_K = 144                  # fsnap::PATH_MAX_K
MAX_CLASS = 8                # fsnap::PATH_MAX_CLASS
PIVOT_TOL = loco.PIVOT_TOL
METHODS = ("auto", "refit", "woodbury")
PATH_SOLVERS = ("RIDGE", "SVD")

RidgePath = namedtuple("RidgePath", ["alphas", "fits", "table", "units", "unidentifiable", "best", "best_alpha", "preds"])


def check_alphas(alphas):
    """The grid as a float64 vector; ValueError when it is empty or holds a negative or non-finite value."""
    alphas = np.asarray(alphas, dtype=np.float64).reshape(-1).copy()
    if alphas.size < 1:
        raise ValueError("ridge_path: the alpha grid is empty")
    if not np.all(np.isfinite(alphas)) or np.any(alphas < 0.0):
        raise ValueError("ridge_path: every alpha must be finite and >= 0")
    return alphas


def row_sums(b, w_eff, pred, rows, row_class, nclass):
    """(nclass x 4) sums n, sum |r|, sum r^2, sum (w r)^2 of r = b - pred over ``rows`` by class."""
    out = np.zeros((nclass, 4))
    r = b[rows] - pred
    cls = row_class[rows]
    for k in range(nclass):
        sel = cls == k
        if sel.any():
            rk = r[sel]
            out[k] = (sel.sum(), np.abs(rk).sum(), (rk * rk).sum(), ((w_eff[rows][sel] * rk) ** 2).sum())
    return out


def ridge_path_host(A, b, w_eff, G, c, alphas, sorted_rows, offsets, row_class=None, nclass=1, tol=PIVOT_TOL):
    """The kernel's closed form in numpy float64 (``np.linalg.solve`` on the scaled downdated system): (sums
    (Q x nunits x nclass x 4), info (Q x nunits x 2: smallest pivot, identifiable), preds (Q x m, NaN where a row is not listed
    or its unit is not identifiable))."""
    A = np.asarray(A, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64).reshape(-1)
    w = np.asarray(w_eff, dtype=np.float64).reshape(-1)
    G = np.asarray(G, dtype=np.float64)
    c = np.asarray(c, dtype=np.float64).reshape(-1)
    alphas = check_alphas(alphas)
    m, K = A.shape
    Q, nunits = alphas.size, len(offsets) - 1
    row_class = np.zeros(m, dtype=np.uint8) if row_class is None else np.asarray(row_class, dtype=np.uint8)
    sums = np.zeros((Q, nunits, nclass, 4))
    info = np.zeros((Q, nunits, 2))
    info[:, :, 0], info[:, :, 1] = np.inf, 1.0
    preds = np.full((Q, m), np.nan)
    eye = np.eye(K)
    for u in range(nunits):
        rows = np.asarray(sorted_rows[offsets[u]:offsets[u + 1]])
        if rows.size == 0:
            continue
        X = A[rows] * w[rows, None]
        base = G - X.T @ X
        r = c - X.T @ (w[rows] * b[rows])
        for q, alpha in enumerate(alphas):
            B = base + alpha * eye
            d = np.diag(B).copy()
            if not (np.all(d > 0.0) and np.all(d > tol * (np.diag(G) + alpha))):
                info[q, u] = (np.min(d) if np.all(np.isfinite(d)) else np.nan, 0.0)
                continue
            s = np.sqrt(d)
            H = B / s[:, None] / s[None, :]
            H[np.diag_indices(K)] = 1.0
            H = np.tril(H) + np.tril(H, -1).T                      # the lower triangle, as the kernel reads it
            try:
                piv = np.diag(np.linalg.cholesky(H)) ** 2
            except np.linalg.LinAlgError:
                piv = loco._cholesky_pivots(H)
            low = np.flatnonzero(~(piv > tol))
            info[q, u, 0] = piv[:low[0] + 1].min() if low.size else piv.min()
            if low.size:
                info[q, u, 1] = 0.0
                continue
            beta = np.linalg.solve(H, r / s) / s
            p = A[rows] @ beta
            preds[q, rows] = p
            sums[q, u] = row_sums(b, w, p, rows, row_class, nclass)
    return sums, info, preds


def ridge_path_woodbury(ctx, b, w_eff, G, c, alphas, sorted_rows, offsets, row_class, nclass):
    """The composed route on the GPU: per alpha ``loco.factor_cholesky`` + ``fsnap_loco_rows`` (the Woodbury form) and the host
    sums.  Same returns as ``ridge_path_host``; info's pivot is that of I - S_u, not of H_q."""
    alphas = check_alphas(alphas)
    b = np.asarray(b, dtype=np.float64).reshape(-1)
    w = np.asarray(w_eff, dtype=np.float64).reshape(-1)
    Q, nunits, m = alphas.size, len(offsets) - 1, b.shape[0]
    sums = np.zeros((Q, nunits, nclass, 4))
    info = np.zeros((Q, nunits, 2))
    preds = np.full((Q, m), np.nan)
    for q, alpha in enumerate(alphas):
        try:
            M = loco.factor_cholesky(G, alpha)
            if M.shape[1] != M.shape[0]:
                raise np.linalg.LinAlgError("zero column")
            beta = M @ (M.T @ np.asarray(c, dtype=np.float64))
        except np.linalg.LinAlgError:
            info[q, :, 0], info[q, :, 1] = np.nan, 0.0             # the fit itself does not exist at this alpha
            continue
        p, inf4 = ctx.loco_rows(M, beta, sorted_rows, offsets)
        preds[q] = p
        info[q, :, 0], info[q, :, 1] = inf4[:, 1], inf4[:, 2]
        for u in range(nunits):
            rows = np.asarray(sorted_rows[offsets[u]:offsets[u + 1]])
            if rows.size and info[q, u, 1]:
                sums[q, u] = row_sums(b, w, p[rows], rows, row_class, nclass)
    return sums, info, preds


def pool_sums(sums, info, keys=None):
    """(Q x nclass x 4) sums over the identifiable units and the count of units that are not identifiable per alpha.  The units
    are added in the order of their keys (as strings; ``keys=None``: as given) by one numpy reduction, so the pooled sums
    have the same bits however the units are dealt to ranks."""
    sums = np.asarray(sums, dtype=np.float64)
    info = np.asarray(info, dtype=np.float64)
    Q, nunits, nclass, _ = sums.shape
    if nunits == 0:
        return np.zeros((Q, nclass, 4)), np.zeros(Q, dtype=np.int64)
    if keys is not None:
        order = sorted(range(nunits), key=lambda i: str(keys[i]))
        sums, info = sums[:, order], info[:, order]
    pooled = np.where(info[:, :, 1, None, None] > 0, sums, 0.0).sum(axis=1)
    return pooled, np.sum(info[:, :, 1] == 0, axis=1).astype(np.int64)


def path_table(alphas, pooled, class_names):
    """DataFrame indexed (alpha, Row_Type) -- one row per class and an ``*ALL`` row per alpha -- with ncount, mae, rmse and
    w_rmse = sqrt(sum (w r)^2 / ncount) from the (Q x nclass x 4) pooled sums."""
    from pandas import DataFrame, MultiIndex

    pooled = np.asarray(pooled, dtype=np.float64)
    index, rows = [], []

    def metrics(s):
        n = s[0]
        if n <= 0:
            return (0, np.nan, np.nan, np.nan)
        return (int(n), s[1] / n, np.sqrt(s[2] / n), np.sqrt(s[3] / n))

    for q, alpha in enumerate(alphas):
        index.append((float(alpha), "*ALL"))
        rows.append(metrics(pooled[q].sum(axis=0)))
        for k, name in enumerate(class_names):
            index.append((float(alpha), name))
            rows.append(metrics(pooled[q, k]))
    return DataFrame(rows, index=MultiIndex.from_tuples(index, names=["alpha", "Row_Type"]),
                     columns=["ncount", "mae", "rmse", "w_rmse"])


def pick_best(alphas, w_sse, unidentifiable):
    """Index of the alpha with the smallest total sum (w r)^2 among the alphas without a unit that is not identifiable; ties
    go to the smaller alpha.  None when no alpha is eligible."""
    alphas = np.asarray(alphas, dtype=np.float64)
    best = None
    for q in range(alphas.size):
        if unidentifiable[q] or not np.isfinite(w_sse[q]):
            continue
        if best is None or w_sse[q] < w_sse[best] or (w_sse[q] == w_sse[best] and alphas[q] < alphas[best]):
            best = q
    return best


def host_fits(G, c, alphas):
    """Q x K: beta_q = (G + alpha_q I)^-1 c through the Jacobi-scaled host solve (NaN where it fails)."""
    from .. import _capi

    G = np.ascontiguousarray(G, dtype=np.float64)
    c = np.ascontiguousarray(c, dtype=np.float64)
    fits = np.full((len(alphas), G.shape[0]), np.nan)
    for q, alpha in enumerate(alphas):
        try:
            fits[q] = _capi.solve(_capi.SOLVE_RIDGE, float(alpha), G, c)[0]
        except (np.linalg.LinAlgError, ValueError):
            pass
    return fits


def check_solver(solver):
    """ValueError unless the solver is a fitted-from-statistics RIDGE or SVD (not ``apply_transpose``, not the row-space path)."""
    kind = type(solver).__name__
    sec = solver.config.sections
    if kind not in PATH_SOLVERS:
        raise ValueError(f"ridge_path: {kind} has no ridge path (only {', '.join(PATH_SOLVERS)} have)")
    if "EXTRAS" in sec and sec["EXTRAS"].apply_transpose:
        raise ValueError("ridge_path: a fit through apply_transpose is a smoother of (G, c), not of the rows")
    if kind == "SVD" and solver.last_row_space is not None:
        raise ValueError("ridge_path: the SVD fit took the row-space path; its statistics are too ill-conditioned for a ridge path")
    return kind


def choose_method(method, K):
    """"refit" (the fused kernel) or "woodbury" (the composed route).  "auto" takes the kernel wherever it exists
    (K <= 144) and the composed route beyond: profiles/ridge_path_timing.txt records both routes at the two shapes
    scripts/ridge_path_timing.py times; a shape class on which the kernel lost would be sent to the composed route here."""
    if method not in METHODS:
        raise ValueError(f"ridge_path: method must be one of {', '.join(METHODS)}")
    if method == "refit" and K > MAX_K:
        raise ValueError(f"ridge_path: method='refit' needs K <= {MAX_K} (K = {K})")
    if method == "auto":
        return "refit" if K <= MAX_K else "woodbury"
    return method


def resolve_rows(solver, who, by, fs_dict=None, b=None, w=None):
    """Labels, truths and weights of the rows of the last fit, as ``loco_errors`` resolves them: ``fs_dict=None`` takes
    ``pt.fitsnap_dict`` (``pt.local_lists`` on several ranks) and the shared ``b`` / ``w``; an explicit ``fs_dict`` needs
    ``b`` and ``w`` (one weight per row, per training row, or one for all).  Returns (labels, b, w, testing mask, sorted
    Row_Type names -- the union over the ranks --, class id per row, number of classes)."""
    pt = solver.pt
    if fs_dict is None:
        labels = pt.local_lists if (pt.multi and getattr(pt, "local_lists", None)) else pt.fitsnap_dict
        b = pt.shared_arrays["b"].array
        w = pt.shared_arrays["w"].array
    elif b is None or w is None:
        raise ValueError(f"{who}: with fs_dict, pass the truths b and weights w of the fit too")
    else:
        labels = fs_dict
    b = np.asarray(b, dtype=np.float64).reshape(-1)
    m = b.shape[0]
    if by not in labels:
        raise KeyError(f"{who}: no '{by}' labels")
    testing = np.asarray(labels["Testing"], dtype=bool) if "Testing" in labels else np.zeros(m, dtype=bool)
    train = ~testing
    w = np.asarray(w, dtype=np.float64).reshape(-1)
    if w.size == 1:
        w = np.full(m, float(w[0]))
    elif w.size == int(train.sum()) and w.size != m:
        wf = np.zeros(m)
        wf[train] = w
        w = wf
    if w.size != m:
        raise ValueError(f"{who}: {w.size} weights for {m} rows")
    if len(labels[by]) != m:
        raise ValueError(f"{who}: {len(labels[by])} '{by}' labels for {m} rows: not the rows of the resident fit")
    rtypes = list(labels["Row_Type"]) if "Row_Type" in labels else ["Row"] * m
    names = sorted(set(rtypes))
    if pt.multi:
        names = sorted({n for part in pt.allgather_object(names) for n in part})
    if len(names) > MAX_CLASS:
        raise ValueError(f"{who}: {len(names)} row types, at most {MAX_CLASS}")
    pos = {n: i for i, n in enumerate(names)}
    row_class = np.fromiter((pos[t] for t in rtypes), dtype=np.uint8, count=m)
    nclass = max(len(names), 1)
    return labels, b, w, testing, names, row_class, nclass


def ridge_path(solver, alphas, by="Configs", fs_dict=None, b=None, w=None, method="auto", want_preds=False):
    """``Solver.ridge_path``: see there."""
    from pandas import DataFrame

    who = "ridge_path"
    pt = solver.pt
    check_solver(solver)                                    # every rank refuses alike
    alphas = check_alphas(alphas)
    if method not in METHODS:
        raise ValueError(f"ridge_path: method must be one of {', '.join(METHODS)}")
    stats = solver.last_statistics if pt._rank == 0 else None
    if pt.multi:
        stats = pt.bcast_object(None if stats is None else (np.asarray(stats[0]), np.asarray(stats[1])), src=0)
    if stats is None:
        raise RuntimeError("ridge_path: call perform_fit first")
    G = np.ascontiguousarray(stats[0], dtype=np.float64)
    c = np.ascontiguousarray(stats[1], dtype=np.float64).reshape(-1)
    K = G.shape[0]
    method = choose_method(method, K)
    labels, b, w, testing, names, row_class, nclass = resolve_rows(solver, who, by, fs_dict, b, w)
    m, train = b.shape[0], ~testing
    sorted_rows, offsets, units = loco.unit_index(labels[by], train)
    if pt.multi:
        try:
            loco.check_units_disjoint(pt.allgather_object(units))
        except ValueError as e:
            raise ValueError(str(e).replace("loco_errors", who)) from None
    ctx = pt.hip() if m > 0 else None
    if m > 0 and (ctx.m != m or ctx.K != K):
        raise ValueError(f"ridge_path: the resident rows ({ctx.m} x {ctx.K}) are not those of the fit ({m} rows, {K} columns)")
    w_eff = np.where(train, w, 0.0)
    if m == 0:
        Q = alphas.size
        sums, info, preds = np.zeros((Q, 0, nclass, 4)), np.zeros((Q, 0, 2)), np.zeros((Q, 0))
    elif method == "refit":
        sums, info, preds = ctx.ridge_path(G, c, alphas, sorted_rows, offsets, row_class, nclass, want_preds=want_preds)
    else:
        sums, info, preds = ridge_path_woodbury(ctx, b, w_eff, G, c, alphas, sorted_rows, offsets, row_class, nclass)
        if not want_preds:
            preds = None
    if preds is not None:
        preds[:, testing] = np.nan
    groups = labels["Groups"] if "Groups" in labels else [None] * m
    urows = [[] for _ in alphas]
    for q, alpha in enumerate(alphas):
        for u, key in enumerate(units):
            rows = sorted_rows[offsets[u]:offsets[u + 1]]
            ident = bool(info[q, u, 1])
            urows[q].append((float(alpha), key, groups[rows[0]] if len(rows) else None, len(rows),
                             float(sums[q, u, :, 3].sum()) if ident else np.nan, ident, float(info[q, u, 0])))
    if pt.multi:
        # the per-unit sums are small (Q x nunits x nclass x 4): gathered and pooled in the order of the unit keys, so that
        # the table does not depend on how the units are spread over the ranks
        parts = pt.allgather_object((np.asarray(sums), np.asarray(info), urows))
        sums = np.concatenate([p[0] for p in parts], axis=1)
        info = np.concatenate([p[1] for p in parts], axis=1)
        urows = [[r for p in parts for r in p[2][q]] for q in range(alphas.size)]
    pooled, bad = pool_sums(sums, info, [r[1] for r in urows[0]])
    urows = [r for part in urows for r in part]
    frame = DataFrame(urows, columns=["alpha", by, "Groups", "rows", "w_sse", "identifiable", "min_pivot"])
    w_sse = pooled[:, :, 3].sum(axis=1)
    best = pick_best(alphas, w_sse, bad)
    fits = host_fits(G, c, alphas) if pt._rank == 0 else None
    table = path_table(alphas, pooled, names)
    return RidgePath(alphas, fits, table, frame, bad, best, None if best is None else float(alphas[best]), preds)
