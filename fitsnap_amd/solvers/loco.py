"""Exact leave-one-configuration-out (LOCO) errors of the linear smoothers (SVD, RIDGE, ANL) without refits.

For the weighted training rows x_i = w_i a_i, y_i = w_i b_i of a fit, G = sum x_i x_i^T and C = (G + alpha I)^-1 = M M^T
(RIDGE: its alpha; ANL: pinv(G + cov_nugget I); SVD: alpha = 0, or the kept directions of a truncated fit; a row-space fit
takes M from the triangle of the rows, ``rows_triangle`` / ``factor_triangle``, since its G is too ill-conditioned),
every row i of a unit c (a configuration, or any label such as a group) has the prediction of the fit without c's rows

    zeta_i = a_i M,  z_i = w_i zeta_i,  e_i = y_i - x_i . beta,  S_c = Z_c^T Z_c
    v_c = (I_J - S_c)^-1 Z_c^T e_c = Z_c^T (I_n - Z_c Z_c^T)^-1 e_c
    p_i = a_i . beta - zeta_i . v_c = a_i . beta_{-c}                 (Woodbury)

The GPU pass is ``fsnap_loco_rows`` (csrc/fsnap_loco.hip); this module builds M and the unit index, holds the same closed
forms in numpy (``loco_host``, the check of the kernel) and turns LOO predictions into ``error_analysis``'s tables.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from .._hostblas import blas_threads

SMOOTHERS = ("SVD", "RIDGE", "ANL")
PIVOT_TOL = 1e-10            # fsnap::LOCO_PIVOT_TOL: pivots of I - S_c at or below it mark a unit that is not identifiable
PINV_RCOND = 1e-15           # numpy.linalg.pinv's default cut (ANL's pinv, anl.py:39)

LocoResult = namedtuple("LocoResult", ["errors", "preds", "units", "unidentifiable"])


def factor_cholesky(G, alpha=0.0):
    """M = D^-1 R^-1 with G + alpha I = D (R^T R) D, D = sqrt(diag(G + alpha I)), so that M M^T = (G + alpha I)^-1.  Columns
    with a zero diagonal (exactly-zero columns of an SVD fit, coefficient 0) get zero rows.  Raises LinAlgError when the
    scaled matrix is not positive definite."""
    G = np.asarray(G, dtype=np.float64)
    K = G.shape[0]
    H = 0.5 * (G + G.T) + float(alpha) * np.eye(K)
    d = np.diag(H).copy()
    keep = d > 0.0
    M = np.zeros((K, K))
    if not keep.any():
        return M
    s = 1.0 / np.sqrt(d[keep])
    Hs = H[np.ix_(keep, keep)] * s[:, None] * s[None, :]
    with blas_threads(Hs.shape[0]):
        L = np.linalg.cholesky(Hs)                              # Hs = L L^T, R = L^T
        Rinv = np.linalg.solve(L, np.eye(L.shape[0])).T          # R^-1 = (L^-1)^T
    sub = s[:, None] * Rinv
    M[np.ix_(keep, keep)] = sub
    return M[:, keep] if not keep.all() else M


def factor_eigen(G, alpha=0.0, rank=None, scaled=True, rcond=PINV_RCOND):
    """M = D^-1 V_r Lambda_r^-1/2 of the largest ``rank`` eigenpairs of D^-1 (G + alpha I) D^-1 (``scaled``; D = I
    otherwise), only eigenvalues above ``rcond`` lambda_max: the pseudo-inverse restricted to the kept directions (a
    truncated SVD fit, ANL's pinv)."""
    G = np.asarray(G, dtype=np.float64)
    K = G.shape[0]
    H = 0.5 * (G + G.T) + float(alpha) * np.eye(K)
    d = np.diag(H).copy()
    keep = d > 0.0 if scaled else np.ones(K, dtype=bool)
    s = 1.0 / np.sqrt(d[keep]) if scaled else np.ones(int(keep.sum()))
    Hs = H[np.ix_(keep, keep)] * s[:, None] * s[None, :]
    with blas_threads(Hs.shape[0]):
        ev, V = np.linalg.eigh(Hs)
    order = np.argsort(ev)[::-1]
    ev, V = ev[order], V[:, order]
    used = ev > rcond * max(ev[0], 0.0) if ev.size else np.zeros(0, dtype=bool)
    if rank is not None:
        used &= np.arange(ev.size) < int(rank)
    r = int(np.count_nonzero(used))
    M = np.zeros((K, max(r, 1)))
    if r:
        M[keep, :r] = s[:, None] * V[:, used] / np.sqrt(ev[used])[None, :]
    return M


def rows_triangle(A, w_eff, parts=None):
    """R of A_w = Q R for the weighted rows A_w = w_eff a (Householder QR on the host); with ``parts`` (the triangles of
    other row blocks, e.g. one per rank) the triangle of all blocks stacked.  R^T R = G without ever forming G."""
    blocks = [] if parts is None else [np.asarray(p, dtype=np.float64) for p in parts]
    if A is not None:
        A = np.asarray(A, dtype=np.float64)
        blocks.append(A * np.asarray(w_eff, dtype=np.float64).reshape(-1, 1))
    stack = np.vstack(blocks)
    if stack.shape[0] == 0:
        return stack
    with blas_threads(stack.shape[1]):
        return np.linalg.qr(stack, mode="r")


def factor_triangle(R, rank=None):
    """M = V_r Sigma_r^-1 of the largest ``rank`` singular triplets of R (A_w = Q R, ``rows_triangle``): M M^T is the
    pseudo-inverse of G on the kept directions and M^T G M = I to kappa(A_w) eps.  The eigenpairs of G itself
    (``factor_eigen``) are good to kappa(A_w)^2 eps only: from kappa ~ 1e8 on, where an SVD fit takes the row-space path,
    the weakest kept column of M would be wrong in its leading digits."""
    R = np.asarray(R, dtype=np.float64)
    K = R.shape[1]
    if R.shape[0] == 0:
        return np.zeros((K, 1))
    with blas_threads(K):
        _, sv, Vt = np.linalg.svd(R, full_matrices=False)
    used = sv > 0.0
    if rank is not None:
        used &= np.arange(sv.size) < int(rank)
    r = int(np.count_nonzero(used))
    M = np.zeros((K, max(r, 1)))
    if r:
        M[:, :r] = Vt[used].T / sv[used][None, :]
    return M


def check_smoother(solver):
    """Kind of a solver whose fit is a linear smoother of the rows; ValueError for any other solver (ARD, LASSO, MERR,
    MCMC) and for fits through ``apply_transpose``."""
    kind = type(solver).__name__
    sec = solver.config.sections
    if kind not in SMOOTHERS:
        raise ValueError(f"loco_errors: {kind} is not a linear smoother of the rows (only {', '.join(SMOOTHERS)} are)")
    if "EXTRAS" in sec and sec["EXTRAS"].apply_transpose:
        raise ValueError("loco_errors: a fit through apply_transpose is a smoother of (G, c), not of the rows")
    return kind


def smoother_factor(solver, triangle=None):
    """(kind, M) of a fitted SVD / RIDGE / ANL solver (on the rank that holds the statistics).  ``triangle``: R of the
    weighted training rows (``rows_triangle``), used for an SVD fit that took the row-space path -- its statistics are too
    ill-conditioned for a factor from G (``factor_triangle``); ``loco_errors`` passes it."""
    kind = check_smoother(solver)
    sec = solver.config.sections
    stats = solver.last_statistics
    if stats is None:
        raise RuntimeError("loco_errors: call perform_fit first")
    G = np.asarray(stats[0], dtype=np.float64)
    K = G.shape[0]
    if kind == "RIDGE":
        alpha = float(sec["RIDGE"].alpha)
        try:
            return kind, factor_cholesky(G, alpha)
        except np.linalg.LinAlgError:
            return kind, factor_eigen(G, alpha)
    if kind == "ANL":
        return kind, factor_eigen(G, float(sec["SOLVER"].cov_nugget), scaled=False)
    # SVD: the fit's own rank decision; a full-rank fit from the statistics inverts G itself
    rank = solver.last_rank
    zero_cols = int(np.count_nonzero(np.diag(G) == 0.0))
    if solver.last_row_space is None and rank is not None and rank >= K:
        try:
            return kind, factor_cholesky(G)
        except np.linalg.LinAlgError:
            pass
    kept = None if rank is None or rank < 0 else min(int(rank), K - zero_cols)
    if solver.last_row_space is not None and triangle is not None:
        return kind, factor_triangle(triangle, rank=kept)
    return kind, factor_eigen(G, 0.0, rank=kept, rcond=0.0)


def unit_index(labels, train):
    """(sorted_rows int32, offsets int64, unit keys) of the training rows grouped by unit label, units in first-seen order,
    rows of a unit in row order (a stable sort)."""
    labels = list(labels)
    train = np.asarray(train, dtype=bool)
    if len(labels) != train.shape[0]:
        raise ValueError(f"{len(labels)} unit labels for {train.shape[0]} rows")
    pos, ids = {}, np.empty(len(labels), dtype=np.int64)
    for i, (lab, t) in enumerate(zip(labels, train)):
        lab = lab.item() if isinstance(lab, np.generic) else lab
        ids[i] = pos.setdefault(lab, len(pos)) if t else -1
    rows = np.flatnonzero(ids >= 0)
    order = np.argsort(ids[rows], kind="stable")
    sorted_rows = rows[order].astype(np.int32)
    counts = np.bincount(ids[rows], minlength=len(pos))
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return sorted_rows, offsets, list(pos)


def check_units_disjoint(parts):
    """ValueError when a unit label occurs in the lists of two ranks (parts: one list of unit labels per rank): the
    closed form needs all of a unit's rows on one GPU."""
    seen = {}
    for r, part in enumerate(parts):
        for u in part:
            if seen.setdefault(u, r) != r:
                raise ValueError(f"loco_errors: unit {u!r} has rows on ranks {seen[u]} and {r}; every unit must live on one "
                                 "rank")


def loco_host(A, b, w_eff, M, beta, sorted_rows, offsets, space="auto", tol=PIVOT_TOL):
    """The kernel's closed form in numpy: (pred (m, NaN where not listed / not identifiable), info (ncfg x 4)).  ``space``:
    "auto" (n space when n_c <= J, as the kernel), "J" or "n"."""
    A = np.asarray(A, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    w = np.asarray(w_eff, dtype=np.float64)
    M = np.asarray(M, dtype=np.float64).reshape(A.shape[1], -1)
    beta = np.asarray(beta, dtype=np.float64).reshape(-1)
    J = M.shape[1]
    pred = np.full(A.shape[0], np.nan)
    info = np.zeros((len(offsets) - 1, 4))
    for c in range(len(offsets) - 1):
        rows = np.asarray(sorted_rows[offsets[c]:offsets[c + 1]])
        n = rows.size
        if n == 0:
            info[c] = (0, np.inf, 1, 1)
            continue
        zeta = A[rows] @ M
        pb = A[rows] @ beta
        Z = w[rows, None] * zeta
        e = w[rows] * b[rows] - w[rows] * pb
        nspace = n <= J if space == "auto" else space == "n"
        H = np.eye(n) - Z @ Z.T if nspace else np.eye(J) - Z.T @ Z
        piv = _cholesky_pivots(H)
        info[c] = (min(n, J), piv.min(), 1.0, 1.0 if nspace else 0.0)
        if not piv.min() > tol:
            info[c, 2] = 0.0
            continue
        v = Z.T @ np.linalg.solve(H, e) if nspace else np.linalg.solve(H, Z.T @ e)
        pred[rows] = pb - zeta @ v
    return pred, info


def _cholesky_pivots(H):
    """Pivots (squared diagonal of the factor before the square root) of an unpivoted Cholesky; stops at the first one that
    is not positive (the rest are reported as that one)."""
    H = np.array(H, dtype=np.float64)
    d = H.shape[0]
    piv = np.empty(d)
    for k in range(d):
        p = H[k, k]
        piv[k:] = p
        if not p > 0.0:
            break
        H[k:, k] /= np.sqrt(p)
        H[k + 1:, k + 1:] -= np.outer(H[k + 1:, k], H[k + 1:, k])
    return piv


def error_sums(solver, truths, preds, weights, groups, row_types):
    """(sorted keys (group, False, row type), (len(keys), 10) sums of fsnap_error_stats) over the rows given."""
    keys = sorted({(g, False, r) for g, r in zip(groups, row_types)})
    pos = {k: i for i, k in enumerate(keys)}
    cat = np.fromiter((pos[(g, False, r)] for g, r in zip(groups, row_types)), dtype=np.int64, count=len(groups))
    return keys, solver._host_error_sums(truths, preds, weights, cat, len(keys))


def loco_errors(solver, by="Configs", fs_dict=None, b=None, w=None):
    """``Solver.loco_errors``: see there."""
    from pandas import DataFrame

    pt = solver.pt
    kind = check_smoother(solver)                           # every rank refuses alike
    fit = solver._uq_inputs()[1]                            # broadcast from rank 0, B0 zeros of _offset taken out
    if fit is None:
        raise RuntimeError("loco_errors: call perform_fit first")
    beta = np.asarray(fit, dtype=np.float64).reshape(-1)
    # the rows, labels, truths and weights of the fit
    if fs_dict is None:
        labels = pt.local_lists if (pt.multi and getattr(pt, "local_lists", None)) else pt.fitsnap_dict
        b = pt.shared_arrays["b"].array
        w = pt.shared_arrays["w"].array
    elif b is None or w is None:
        raise ValueError("loco_errors: with fs_dict, pass the truths b and weights w of the fit too")
    else:
        labels = fs_dict
    b = np.asarray(b, dtype=np.float64).reshape(-1)
    m = b.shape[0]
    if by not in labels:
        raise KeyError(f"loco_errors: no '{by}' labels")
    testing = np.asarray(labels["Testing"], dtype=bool) if "Testing" in labels else np.zeros(m, dtype=bool)
    train = ~testing
    w = np.asarray(w, dtype=np.float64).reshape(-1)
    if w.size == 1:
        w = np.full(m, float(w[0]))
    elif w.size == int(train.sum()) and w.size != m:       # one weight per training row, as perform_fit takes them
        wf = np.zeros(m)
        wf[train] = w
        w = wf
    if w.size != m:
        raise ValueError(f"loco_errors: {w.size} weights for {m} rows")
    sorted_rows, offsets, units = unit_index(labels[by], train)
    if pt.multi:
        check_units_disjoint(pt.allgather_object(units))
    ctx = pt.hip() if m > 0 else None
    if m > 0 and (ctx.m != m or ctx.K != beta.shape[0]):
        raise RuntimeError(f"loco_errors: the resident rows ({ctx.m} x {ctx.K}) are not those of the fit ({m} rows, "
                           f"{beta.shape[0]} columns): call perform_fit first")
    triangle = None
    if kind == "SVD" and solver.last_row_space is not None:
        # a fit on the rows (every rank took that path): M from the rows too, through their triangle
        triangle = rows_triangle(ctx.download_rows(want_b=False, want_w=False)[0] if m > 0 else np.zeros((0, beta.shape[0])),
                                 np.where(train, w, 0.0))
        if pt.multi:
            triangle = rows_triangle(None, None, pt.allgather_object(triangle))
    M = smoother_factor(solver, triangle)[1] if pt._rank == 0 else None
    if pt.multi:
        M = pt.bcast_object(M, src=0)
    if m > 0:
        preds, info = ctx.loco_rows(M, beta, sorted_rows, offsets)
    else:
        preds, info = np.zeros(0), np.zeros((0, 4))
    preds[testing] = np.nan
    # tables over the training rows of identifiable units, from the LOO predictions
    groups = labels["Groups"]
    rtypes = labels["Row_Type"]
    ok = np.flatnonzero(train & np.isfinite(preds))
    keys, st = error_sums(solver, b[ok], preds[ok], w[ok], [groups[i] for i in ok], [rtypes[i] for i in ok])
    # per-unit frame
    res = b - preds
    urows = []
    for u, key in enumerate(units):
        rows = sorted_rows[offsets[u]:offsets[u + 1]]
        ident = bool(info[u, 2]) if len(rows) else True
        urows.append((key, groups[rows[0]], len(rows), float(np.sum((w[rows] * res[rows]) ** 2)) if ident else np.nan,
                      float(np.max(np.abs(res[rows]))) if ident and len(rows) else np.nan, ident, int(info[u, 0]),
                      float(info[u, 1])))
    if pt.multi:
        gkeys = sorted({k for part in pt.allgather_object(list(keys)) for k in part})
        table = np.zeros((len(gkeys), 10))
        if len(keys):
            pos = {k: i for i, k in enumerate(gkeys)}
            table[[pos[k] for k in keys]] = np.asarray(st, dtype=np.float64).reshape(len(keys), 10)
        tables = solver._allgather_tables(table)
        urows = [r for part in pt.allgather_object(urows) for r in part]
        keys = gkeys
        st = np.array([solver._pool_sums(rows[rows[:, 0] > 0]) for rows in np.swapaxes(tables, 0, 1)]).reshape(len(gkeys), 10)
    nbad = sum(1 for r in urows if not r[5])
    frame = DataFrame(urows, columns=[by, "Groups", "rows", "w_sse", "max_abs_res", "identifiable", "d", "min_pivot"])
    if pt._rank != 0:
        return LocoResult(None, preds, frame, nbad)
    if not keys:
        return LocoResult(None, preds, frame, nbad)
    grouped, allrows = solver._tables_from_sums(keys, st)
    return LocoResult(solver._assemble_errors(grouped, allrows, None), preds, frame, nbad)
