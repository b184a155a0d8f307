"""Per-configuration influence on the coefficients and cluster-robust coefficient covariances of the linear smoothers (SVD,
RIDGE, ANL), no refits.

With the conventions of ``loco`` (C = (G + alpha I)^-1 = M M^T, zeta_i = a_i M, z_i = w_i zeta_i, e_i = w_i b_i - w_i a_i . beta),
a unit c (a configuration, or any label) has

    s_c = Z_c^T e_c                         the score of the unit in M space
    v_c = (I - Z_c^T Z_c)^-1 s_c            ``loco``'s v: the refit without c is beta_{-c} = beta - M v_c, exactly
    W_s = sum_c s_c s_c^T,  W_v = sum_{c identifiable} v_c v_c^T

and with U the units that have a row of w > 0, U' the identifiable ones among them, n the training rows with w > 0,
p = tr(G C) and sigma^2 the noise of a unit-weight row (``loco_uq.resolve_noise``):

    cov_classical = sigma^2 C                                 independent rows
    cov_cr0  = M W_s M^T                                      cluster-robust ("sandwich"), clusters = units
    cov_cr1  = U / (U - 1) (n - 1) / (n - p) cov_cr0          its small-sample form
    cov_jack = (U' - 1) / U' M W_v M^T                        CR3: the delete-one-unit jackknife, uncentred around the full fit
    cook_c   = |v_c|^2 / (p sigma^2)                          = dbeta_c^T (G + alpha I) dbeta_c / (p sigma^2), M^T C^+ M = I
    dfbeta   = -V M^T  (units x K),  dfbetas = dfbeta / sqrt(diag cov_classical)

The GPU pass is ``fsnap_influence_rows`` (csrc/fsnap_influence.hip); this module holds the same closed forms in numpy
(``influence_host``, the check of the kernel and the ``method="host"`` route), the covariances and the tables.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from . import loco, loco_uq

SCORES, FULL = 0, 1          # fsnap_influence_rows modes (_capi.INFL_SCORES, _capi.INFL_FULL)
KINDS = ("cr0", "cr1", "jack")
UNIT_COLUMNS = ["Groups", "rows", "rows_weighted", "identifiable", "d", "min_pivot", "cook", "shift", "score"]

InfluenceResult = namedtuple("InfluenceResult", ["units", "cov", "stderr", "dfbeta", "noise", "unidentifiable"])


def influence_host(A, b, w_eff, M, beta, sorted_rows, offsets, mode=FULL, tol=loco.PIVOT_TOL):
    """The kernel's closed form in numpy, a dict as ``HipContext.influence_rows`` returns it: "info" (ncfg x 4: d_c, smallest
    pivot, identifiable, n space; SCORES: d_c, inf, 1, n space), "unit" (ncfg x 3: |v_c|^2, |s_c|^2, s_c . v_c; the first and
    third NaN where c is not identifiable and in SCORES mode; zeros for a unit without rows), "S" (ncfg x J), "Ws" (J x J) and,
    in FULL mode, "pred" (m, as ``loco_host``), "V" (ncfg x J, zeros where c is not identifiable) and "Wv" (None in SCORES)."""
    A = np.asarray(A, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    w = np.asarray(w_eff, dtype=np.float64)
    M = np.asarray(M, dtype=np.float64).reshape(A.shape[1], -1)
    beta = np.asarray(beta, dtype=np.float64).reshape(-1)
    if mode not in (SCORES, FULL):
        raise ValueError(f"mode {mode!r} (SCORES, FULL)")
    full = mode == FULL
    J = M.shape[1]
    ncfg = len(offsets) - 1
    pred = np.full(A.shape[0], np.nan) if full else None
    info = np.zeros((ncfg, 4))
    unit = np.zeros((ncfg, 3))
    S = np.zeros((ncfg, J))
    V = np.zeros((ncfg, J)) if full else None
    for c in range(ncfg):
        rows = np.asarray(sorted_rows[offsets[c]:offsets[c + 1]])
        n = rows.size
        nspace = n <= J
        info[c] = (min(n, J), np.inf, 1.0, 1.0 if nspace else 0.0)
        if n == 0:
            continue
        zeta = A[rows] @ M
        pb = A[rows] @ beta
        Z = w[rows, None] * zeta
        e = w[rows] * b[rows] - w[rows] * pb
        S[c] = Z.T @ e
        unit[c] = (np.nan, S[c] @ S[c], np.nan)
        if not full:
            continue
        H = np.eye(n) - Z @ Z.T if nspace else np.eye(J) - Z.T @ Z
        piv = loco._cholesky_pivots(H)
        info[c, 1] = piv.min()
        if not piv.min() > tol:
            info[c, 2] = 0.0
            continue
        V[c] = Z.T @ np.linalg.solve(H, e) if nspace else np.linalg.solve(H, S[c])
        pred[rows] = pb - zeta @ V[c]
        unit[c, 0] = V[c] @ V[c]
        unit[c, 2] = S[c] @ V[c]
    return {"pred": pred, "info": info, "unit": unit, "S": S, "V": V, "Ws": S.T @ S, "Wv": V.T @ V if full else None}


def unit_counts(w, sorted_rows, offsets, info):
    """(rows with w > 0 per unit, U, U', n): U the units with such a row, U' the identifiable ones among them, n their rows."""
    w = np.asarray(w, dtype=np.float64)
    live = np.array([int(np.count_nonzero(w[sorted_rows[offsets[u]:offsets[u + 1]]] > 0.0)) for u in range(len(offsets) - 1)],
                    dtype=np.int64)
    has = live > 0
    return live, int(has.sum()), int((has & (np.asarray(info)[:, 2] != 0.0)).sum()), int(live.sum())


def covariances(M, Ws, Wv, noise, U, Uid, n, p, kinds=("cr1", "jack")):
    """dict of K x K covariances: ``classical`` = noise M M^T and the ``kinds`` asked for (``cr0``, ``cr1``, ``jack``: see the
    module text).  ``cr1`` is NaN when U < 2 or n <= p, ``jack`` when there is no identifiable unit."""
    M = np.asarray(M, dtype=np.float64)
    out = {"classical": float(noise) * (M @ M.T)}
    for kind in kinds:
        if kind not in KINDS:
            raise ValueError(f"influence: kind {kind!r} ({', '.join(KINDS)})")
    if "cr0" in kinds or "cr1" in kinds:
        cr0 = M @ np.asarray(Ws, dtype=np.float64) @ M.T
        cr0 = 0.5 * (cr0 + cr0.T)
        if "cr0" in kinds:
            out["cr0"] = cr0
        if "cr1" in kinds:
            out["cr1"] = (U / (U - 1.0)) * ((n - 1.0) / (n - p)) * cr0 if U > 1 and n > p else np.full_like(cr0, np.nan)
    if "jack" in kinds:
        jk = M @ np.asarray(Wv, dtype=np.float64) @ M.T
        out["jack"] = ((Uid - 1.0) / Uid) * 0.5 * (jk + jk.T) if Uid > 0 else np.full_like(jk, np.nan)
    return out


def stderr_frame(beta, cov):
    """DataFrame per coefficient: beta, ``se_<kind>`` of every covariance of ``cov`` and ``ratio_<kind>`` = se_<kind> /
    se_classical for the others."""
    from pandas import DataFrame

    cols = {"beta": np.asarray(beta, dtype=np.float64).reshape(-1)}
    with np.errstate(invalid="ignore", divide="ignore"):
        se = {k: np.sqrt(np.diag(c)) for k, c in cov.items()}
        for k, v in se.items():
            cols["se_" + k] = v
        for k, v in se.items():
            if k != "classical":
                cols["ratio_" + k] = v / se["classical"]
    return DataFrame(cols)


def unit_records(units, groups, live, sorted_rows, offsets, info, unit, noise, p):
    """One record per unit, columns ``UNIT_COLUMNS`` after the label: group, rows, rows with w > 0, identifiable, d, smallest
    pivot, Cook's distance |v_c|^2 / (p sigma^2), shift = |v_c|^2 and score = |s_c|^2 (cook and shift NaN where v_c is not
    known: units that are not identifiable, and every unit of a scores-only pass)."""
    out = []
    for u, key in enumerate(units):
        rows = sorted_rows[offsets[u]:offsets[u + 1]]
        shift = float(unit[u, 0])
        out.append((key, groups[rows[0]] if len(rows) else None, len(rows), int(live[u]), bool(info[u, 2]), int(info[u, 0]),
                    float(info[u, 1]), shift / (p * noise) if p > 0 else np.nan, shift, float(unit[u, 1])))
    return out


def influence(solver, by="Configs", fs_dict=None, b=None, w=None, kinds=("cr1", "jack"), noise=None, want_dfbeta=False,
              method="auto"):
    """``Solver.influence``: see there."""
    from pandas import DataFrame

    from . import ridge_path

    who = "influence"
    pt = solver.pt
    try:
        kind = loco.check_smoother(solver)                  # every rank refuses alike
    except ValueError as e:
        raise ValueError(str(e).replace("loco_errors", who)) from None
    if method not in ("auto", "device", "host"):
        raise ValueError(f"{who}: method {method!r} (auto, device, host)")
    kinds = tuple(kinds)
    for k in kinds:
        if k not in KINDS:
            raise ValueError(f"{who}: kind {k!r} ({', '.join(KINDS)})")
    mode = FULL if ("jack" in kinds or want_dfbeta) else SCORES      # v_c (cook, shift, dfbeta, jack) needs the factorisations
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
        p = loco_uq.smoother_trace(solver.last_statistics[0], M)
        try:
            shared = (M, p, loco_uq.resolve_noise(kind, noise, solver.sigmahat, solver.last_statistics, beta, M), None)
        except ValueError as e:                             # every rank refuses alike
            shared = (M, p, None, str(e).replace("loco_predictive", who))
    if pt.multi:
        shared = pt.bcast_object(shared, src=0)
    M, p, noise, refused = shared
    if refused:
        raise ValueError(refused)
    J = M.shape[1]
    w_eff = np.where(train, w, 0.0)
    if m == 0:
        out = {"info": np.zeros((0, 4)), "unit": np.zeros((0, 3)), "V": np.zeros((0, J)), "Ws": np.zeros((J, J)),
               "Wv": np.zeros((J, J))}
    elif method == "host":
        out = influence_host(ctx.download_rows(want_b=False, want_w=False)[0], b, w_eff, M, beta, sorted_rows, offsets, mode)
    else:
        out = ctx.influence_rows(M, beta, sorted_rows, offsets, mode=mode, want_pred=False,
                                 want_vectors=bool(want_dfbeta) and mode == FULL)
    live, U, Uid, n = unit_counts(w_eff, sorted_rows, offsets, out["info"])
    Ws = np.ascontiguousarray(out["Ws"], dtype=np.float64)
    Wv = np.ascontiguousarray(out["Wv"], dtype=np.float64) if mode == FULL else np.zeros((J, J))
    urows = unit_records(units, labels["Groups"], live, sorted_rows, offsets, out["info"], out["unit"], noise, p)
    if pt.multi:
        packed = np.ascontiguousarray(np.concatenate([Ws.reshape(-1), Wv.reshape(-1), [U, Uid, n]]))
        pt.allreduce_host(packed, 0)
        Ws, Wv = packed[:J * J].reshape(J, J), packed[J * J:2 * J * J].reshape(J, J)
        U, Uid, n = (int(round(x)) for x in packed[2 * J * J:])
        urows = [r for part in pt.allgather_object(urows) for r in part]
    frame = DataFrame(urows, columns=[by] + UNIT_COLUMNS)
    nbad = sum(1 for r in urows if not r[4])
    dfbeta = -(np.asarray(out["V"]) @ M.T) if want_dfbeta else None      # this rank's units, in the order of its frame rows
    if pt._rank != 0:
        return InfluenceResult(frame, None, None, dfbeta, noise, nbad)
    cov = covariances(M, Ws, Wv, noise, U, Uid, n, p, kinds)
    return InfluenceResult(frame, cov, stderr_frame(beta, cov), dfbeta, noise, nbad)
