"""Leave-one-configuration-out predictive variances and calibration of the linear smoothers (SVD, RIDGE, ANL), no refits.

With the conventions of ``loco`` (C = (G + alpha I)^-1 = M M^T, zeta_i = a_i M, z_i = w_i zeta_i, e_i = w_i b_i - w_i a_i . beta)
a unit c of n rows has H_c = I - Z_c Z_c^T (n space, n <= J) or I - Z_c^T Z_c (J space) = L L^T, and H_c^-1 is the predictive
covariance of the unit's weighted rows under the fit without the unit, in units of the noise:

    q_i = a_i (G - X_c^T X_c + alpha I)^-1 a_i^T          the leave-out leverage of the unweighted row
        = |L^-1 zeta_i^T|^2                                          (J space)
        = |zeta_i|^2 + |L^-1 g_i|^2,  g_i = Z_c zeta_i^T             (n space; never (H^-1)_ii - 1, which cancels)
    D_c = e_c^T H_c^-1 e_c   = e_c . u  (n space)  = |e_c|^2 + (Z_c^T e_c) . v  (J space)
    l_c = log det H_c = 2 sum log L_kk                               (the same number in either space, Sylvester)

With the noise variance sigma^2 of a unit-weight row: Var(b_i - p_i) = sigma^2 (1 / w_i^2 + q_i), the standardised residual
z_i = w_i (b_i - p_i) / (sigma sqrt(1 + w_i^2 q_i)), and the joint log density of the unit's targets b_c under the fit without it

    -1/2 [n' log(2 pi sigma^2) - l_c + D_c / sigma^2] + sum log w_i          (n' and the sum: the rows with w_i > 0)

whose sum over the units is the exact leave-one-configuration-out log predictive density.  The GPU pass is
``fsnap_loco_rows_uq`` (csrc/fsnap_loco_uq.hip); this module holds the same closed forms in numpy (``loco_uq_host``, the
baseline and the check of the kernel), the noise resolution, and the tables.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from . import loco

NOMINAL_1 = 0.6827           # P(|z| <= 1) and P(|z| <= 2) of a standard normal
NOMINAL_2 = 0.9545
TABLE_COLUMNS = ["n", "mean_z2", "within_1", "nominal_1", "within_2", "nominal_2", "nlpd"]
UNIT_COLUMNS = ["Groups", "rows", "rows_weighted", "d", "identifiable", "distance", "logdet", "logdens"]

LocoPredictive = namedtuple("LocoPredictive", ["pred", "leverage", "var", "z", "units", "tables", "summary", "noise"])


def loco_uq_host(A, b, w_eff, M, beta, sorted_rows, offsets, space="auto", tol=loco.PIVOT_TOL):
    """The kernel's closed form in numpy: (pred (m), leverage q (m), info (ncfg x 6: d_c, smallest pivot, identifiable, n
    space, l_c, D_c)).  pred and q are NaN where a row is not listed or its unit is not identifiable (l_c, D_c NaN too); an
    empty unit gets (0, inf, 1, 1, 0, 0).  ``space``: "auto" (n space when n_c <= J, as the kernel), "J" or "n"."""
    A = np.asarray(A, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    w = np.asarray(w_eff, dtype=np.float64)
    M = np.asarray(M, dtype=np.float64).reshape(A.shape[1], -1)
    beta = np.asarray(beta, dtype=np.float64).reshape(-1)
    J = M.shape[1]
    pred = np.full(A.shape[0], np.nan)
    lev = np.full(A.shape[0], np.nan)
    info = np.zeros((len(offsets) - 1, 6))
    for c in range(len(offsets) - 1):
        rows = np.asarray(sorted_rows[offsets[c]:offsets[c + 1]])
        n = rows.size
        if n == 0:
            info[c] = (0, np.inf, 1, 1, 0, 0)
            continue
        zeta = A[rows] @ M
        pb = A[rows] @ beta
        wc = w[rows]
        Z = wc[:, None] * zeta
        e = wc * b[rows] - wc * pb
        nspace = n <= J if space == "auto" else space == "n"
        H = np.eye(n) - Z @ Z.T if nspace else np.eye(J) - Z.T @ Z
        piv = loco._cholesky_pivots(H)
        info[c] = (min(n, J), piv.min(), 1.0, 1.0 if nspace else 0.0, np.nan, np.nan)
        if not piv.min() > tol:
            info[c, 2] = 0.0
            continue
        L = np.linalg.cholesky(H)
        if nspace:
            u = np.linalg.solve(H, e)
            v = Z.T @ u
            gram = zeta @ zeta.T
            Y = np.linalg.solve(L, wc[:, None] * gram)         # column i: L^-1 g_i, g_i = Z_c zeta_i^T = W gram[:, i]
            lev[rows] = np.diag(gram) + np.sum(Y * Y, axis=0)
            dist = e @ u
        else:
            rhs = Z.T @ e
            v = np.linalg.solve(H, rhs)
            Y = np.linalg.solve(L, zeta.T)
            lev[rows] = np.sum(Y * Y, axis=0)
            dist = e @ e + rhs @ v
        pred[rows] = pb - zeta @ v
        info[c, 4] = 2.0 * np.sum(np.log(np.diag(L)))
        info[c, 5] = dist
    return pred, lev, info


def smoother_trace(G, M):
    """tr(G C) = tr(M^T G M) of C = M M^T: the degrees of freedom the fit spends (K without a ridge, less with one)."""
    G = np.asarray(G, dtype=np.float64)
    M = np.asarray(M, dtype=np.float64).reshape(G.shape[0], -1)
    return float(np.sum(M * (G @ M)))


def resolve_noise(kind, noise, sigmahat, stats, beta, M):
    """sigma^2 of a unit-weight row.  An explicit ``noise`` wins; ANL: ``sigmahat``; SVD / RIDGE: the weighted residual sum of
    squares of the fit, s_0 - 2 beta . c + beta^T G beta from the statistics (G, c, (bw . bw, sum bw, n_train)), over
    n_train - tr(G C).  ValueError when the value is not positive and finite or that denominator is not positive."""
    if noise is None and kind == "ANL":
        noise = sigmahat
        if noise is None:
            raise RuntimeError("loco_predictive: call perform_fit first")
    if noise is None:
        G, c, s = stats
        G = np.asarray(G, dtype=np.float64)
        beta = np.asarray(beta, dtype=np.float64).reshape(-1)
        dof = float(s[2]) - smoother_trace(G, M)
        if not dof > 0.0:
            raise ValueError(f"loco_predictive: {float(s[2]):g} training rows leave {dof:g} degrees of freedom for the noise; "
                             "pass noise=")
        rss = float(s[0]) - 2.0 * float(beta @ np.asarray(c, dtype=np.float64)) + float(beta @ (G @ beta))
        noise = max(rss, 0.0) / dof
    noise = float(noise)
    if not (np.isfinite(noise) and noise > 0.0):
        raise ValueError(f"loco_predictive: the noise variance {noise!r} is not positive")
    return noise


def row_stats(b, w, pred, lev, noise):
    """(var, z, nlpd) per row: Var(b_i - p_i) = sigma^2 (1 / w_i^2 + q_i), z_i = w_i (b_i - p_i) / (sigma sqrt(1 + w_i^2 q_i))
    and the marginal negative log density of b_i, 1/2 [log(2 pi var_i) + (b_i - p_i)^2 / var_i].  NaN where pred or q is (rows
    not listed, testing rows, units that are not identifiable) and where w_i = 0 (no noise model for the row)."""
    b, w, pred, lev = (np.asarray(x, dtype=np.float64) for x in (b, w, pred, lev))
    ok = np.isfinite(pred) & np.isfinite(lev) & (w > 0.0)
    var, z, nlpd = (np.full(b.shape, np.nan) for _ in range(3))
    wk, res = w[ok], b[ok] - pred[ok]
    scale = 1.0 + wk * wk * lev[ok]
    var[ok] = noise * scale / (wk * wk)
    z[ok] = wk * res / np.sqrt(noise * scale)
    nlpd[ok] = 0.5 * (np.log(2.0 * np.pi * var[ok]) + z[ok] ** 2)
    return var, z, nlpd


def unit_records(units, groups, w, sorted_rows, offsets, info, noise):
    """One record per unit, columns ``UNIT_COLUMNS`` after the label: group, rows, rows with w > 0 (n'), d, identifiable,
    D_c / sigma^2, l_c and the joint log density of the unit's targets b_c (NaN for a unit that is not identifiable)."""
    w = np.asarray(w, dtype=np.float64)
    out = []
    for u, key in enumerate(units):
        rows = sorted_rows[offsets[u]:offsets[u + 1]]
        ident = bool(info[u, 2])
        wpos = w[rows][w[rows] > 0.0]
        dist, logdet = (float(info[u, 5]) / noise, float(info[u, 4])) if ident else (np.nan, np.nan)
        logdens = -0.5 * (wpos.size * np.log(2.0 * np.pi * noise) - logdet + dist) + float(np.sum(np.log(wpos)))
        out.append((key, groups[rows[0]] if len(rows) else None, len(rows), int(wpos.size), int(info[u, 0]), ident, dist,
                    logdet, logdens))
    return out


def table_sums(z, nlpd, groups, row_types):
    """(sorted keys (group, row type), (len(keys), 5) sums: n, sum z^2, count |z| <= 1, count |z| <= 2, sum nlpd) over the rows
    with a finite z.  Sums of rows pool by addition (several ranks)."""
    z = np.asarray(z, dtype=np.float64)
    ok = np.flatnonzero(np.isfinite(z))
    keys = sorted({(groups[i], row_types[i]) for i in ok})
    pos = {k: i for i, k in enumerate(keys)}
    st = np.zeros((len(keys), 5))
    if ok.size:
        cat = np.fromiter((pos[(groups[i], row_types[i])] for i in ok), dtype=np.int64, count=ok.size)
        zz = z[ok]
        for col, val in enumerate((np.ones(ok.size), zz * zz, np.abs(zz) <= 1.0, np.abs(zz) <= 2.0,
                                   np.asarray(nlpd, dtype=np.float64)[ok])):
            st[:, col] = np.bincount(cat, weights=val, minlength=len(keys))
    return keys, st


def tables_frame(keys, st):
    """DataFrame indexed (Group, Row_Type), columns ``TABLE_COLUMNS``: the ``*ALL`` rows first (every row type pooled over the
    groups, then (``*ALL``, ``*ALL``) over everything), then one row per (group, row type)."""
    from pandas import DataFrame, MultiIndex

    st = np.asarray(st, dtype=np.float64).reshape(len(keys), 5)
    index, sums = [], []
    for rt in sorted({k[1] for k in keys}):
        index.append(("*ALL", rt))
        sums.append(st[[i for i, k in enumerate(keys) if k[1] == rt]].sum(axis=0))
    index.append(("*ALL", "*ALL"))
    sums.append(st.sum(axis=0))
    index += list(keys)
    sums = np.vstack(sums + [st])
    n = sums[:, 0]
    with np.errstate(invalid="ignore", divide="ignore"):
        per = sums[:, 1:] / n[:, None]
    frame = DataFrame({"n": n.astype(np.int64), "mean_z2": per[:, 0], "within_1": per[:, 1], "nominal_1": NOMINAL_1,
                       "within_2": per[:, 2], "nominal_2": NOMINAL_2, "nlpd": per[:, 3]},
                      index=MultiIndex.from_tuples(index, names=["Group", "Row_Type"]))
    return frame[TABLE_COLUMNS]


def summary(unit_rows, st):
    """dict: ``logdens`` (the total leave-out log predictive density: the sum of the identifiable units' joint log densities),
    ``mean_z2`` (over the rows of ``st``, the sums of ``table_sums``), ``calibrated_noise`` in units of the noise used
    (sum D_c / sigma^2 over sum n'_c of the identifiable units: multiply by sigma^2 for the sigma^2 at which the joint chi^2
    matches its degrees of freedom -- ``loco_predictive`` does), ``units`` and ``unidentifiable``."""
    st = np.asarray(st, dtype=np.float64).reshape(-1, 5)
    good = [r for r in unit_rows if r[5]]
    nprime = sum(r[3] for r in good)
    n = float(st[:, 0].sum())
    return {"logdens": float(sum(r[8] for r in good)),
            "mean_z2": float(st[:, 1].sum()) / n if n else np.nan,
            "calibrated_noise": float(sum(r[6] for r in good)) / nprime if nprime else np.nan,
            "units": len(unit_rows), "unidentifiable": len(unit_rows) - len(good)}


def loco_predictive(solver, by="Configs", fs_dict=None, b=None, w=None, noise=None, method="auto"):
    """``Solver.loco_predictive``: see there."""
    from pandas import DataFrame

    from . import ridge_path

    who = "loco_predictive"
    pt = solver.pt
    try:
        kind = loco.check_smoother(solver)                  # every rank refuses alike
    except ValueError as e:
        raise ValueError(str(e).replace("loco_errors", who)) from None
    if method not in ("auto", "device", "host"):
        raise ValueError(f"{who}: method {method!r} (auto, device, host)")
    fit = solver._uq_inputs()[1]                            # broadcast from rank 0, B0 zeros of _offset taken out
    if fit is None:
        raise RuntimeError(f"{who}: call perform_fit first")
    beta = np.asarray(fit, dtype=np.float64).reshape(-1)
    labels, b, w, testing = ridge_path.resolve_rows(solver, who, by, fs_dict, b, w)[:4]
    m = b.shape[0]
    train = ~testing
    sorted_rows, offsets, units = loco.unit_index(labels[by], train)
    if pt.multi:
        try:
            loco.check_units_disjoint(pt.allgather_object(units))
        except ValueError as e:
            raise ValueError(str(e).replace("loco_errors", who)) from None
    ctx = pt.hip() if m > 0 else None
    if m > 0 and (ctx.m != m or ctx.K != beta.shape[0]):
        raise RuntimeError(f"{who}: the resident rows ({ctx.m} x {ctx.K}) are not those of the fit ({m} rows, "
                           f"{beta.shape[0]} columns): call perform_fit first")
    triangle = None
    if kind == "SVD" and solver.last_row_space is not None:
        triangle = loco.rows_triangle(ctx.download_rows(want_b=False, want_w=False)[0] if m > 0
                                      else np.zeros((0, beta.shape[0])), np.where(train, w, 0.0))
        if pt.multi:
            triangle = loco.rows_triangle(None, None, pt.allgather_object(triangle))
    shared = None
    if pt._rank == 0:
        M = loco.smoother_factor(solver, triangle)[1]
        try:
            shared = (M, resolve_noise(kind, noise, solver.sigmahat, solver.last_statistics, beta, M), None)
        except ValueError as e:                             # every rank refuses alike
            shared = (M, None, str(e))
    if pt.multi:
        shared = pt.bcast_object(shared, src=0)
    M, noise, refused = shared
    if refused:
        raise ValueError(refused)
    if m == 0:
        pred, lev, info = np.zeros(0), np.zeros(0), np.zeros((0, 6))
    elif method == "host":
        pred, lev, info = loco_uq_host(ctx.download_rows(want_b=False, want_w=False)[0], b, np.where(train, w, 0.0), M, beta,
                                       sorted_rows, offsets)
    else:
        pred, lev, info = ctx.loco_rows_uq(M, beta, sorted_rows, offsets)
    pred[testing] = np.nan
    lev[testing] = np.nan
    var, z, nlpd = row_stats(b, w, pred, lev, noise)
    rtypes = labels["Row_Type"] if "Row_Type" in labels else ["Row"] * m
    keys, st = table_sums(z, nlpd, labels["Groups"], rtypes)
    urows = unit_records(units, labels["Groups"], w, sorted_rows, offsets, info, noise)
    if pt.multi:
        parts = pt.allgather_object((keys, st, urows))
        keys = sorted({k for part in parts for k in part[0]})
        pos = {k: i for i, k in enumerate(keys)}
        st = np.zeros((len(keys), 5))
        for pk, ps, _ in parts:
            for k, row in zip(pk, ps):
                st[pos[k]] += row
        urows = [r for part in parts for r in part[2]]
    frame = DataFrame(urows, columns=[by] + UNIT_COLUMNS)
    if pt._rank != 0:
        return LocoPredictive(pred, lev, var, z, frame, None, None, noise)
    out = summary(urows, st)
    out["calibrated_noise"] *= noise
    return LocoPredictive(pred, lev, var, z, frame, tables_frame(keys, st), out, noise)
