"""Robust M-estimator fits by iteratively re-weighted least squares (IRLS) on the GPU, the ``ROBUST`` plugin solver and the
numpy yardstick of the iteration.  No counterpart in the reference: every solver there minimises a squared loss.

The algorithm (fixed; tests/robust_cases.py restates it in long double).  Participating rows are the training rows with
w_i > 0; every other row takes no part in any sum, median or count::

    beta_0 = the ordinary fit with weights w and ridge term alpha, or a caller-supplied start
    for t = 0 .. max_iter - 1:
        e_i = w_i (b_i - a_i . beta_t)
        if t < scale_iters or scale_iters == 0:      s_g = 1.4826 median{|e_i| : class g}   (numpy's median)
        r_i = sqrt(omega(e_i / s_g(i)))              s_g == 0 or an empty class: r_i = 1
        beta_{t+1} = argmin sum (w_i r_i)^2 (b_i - a_i . beta)^2 + alpha |beta|^2
        converged when max |beta_{t+1} - beta_t| <= tol max |beta_{t+1}|

with r formed without the square root of a difference, the branch decided on |e| against the single product c s::

    huber     (c = 1.345)   r = 1 if |e| <= c s else sqrt((c s) / |e|)      rho = u^2 / 2 ; c |u| - c^2 / 2
    bisquare  (c = 4.685)   r = 1 - (e / (c s))^2 if |e| < c s else 0       rho = c^2 / 6 (1 - (1 - (u / c)^2)^3) ; c^2 / 6
    cauchy    (c = 2.385)   r = 1 / sqrt(1 + (e / (c s))^2)                 rho = c^2 / 2 log(1 + (u / c)^2)

(u = e / s; a class without a scale contributes rho = 0).  On the GPU route (``robust_fit``) the step between two fits runs in
csrc/fsnap_robust.hip through the ``fsnap_robust_*`` session: no m-length vector crosses the bus, the fit of every iteration
is the context's own statistics -> solve path reading w_i r_i.  ``robust_host`` is the same iteration in numpy fp64."""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

from .. import _capi
from .solver import Solver

DEFAULT_TUNE = {"huber": 1.345, "bisquare": 4.685, "cauchy": 2.385}
MAD_TO_SIGMA = 1.4826
TABLE_COLUMNS = ("n", "downweighted", "rejected", "sum_omega", "sum_e2", "sum_rho")


def resolve_loss(loss, tune):
    """(loss name, tuning constant): the name checked, ``tune=None`` replaced by the loss's default."""
    name = str(loss).strip().lower()
    if name not in DEFAULT_TUNE:
        raise ValueError(f"unknown loss {loss!r}: one of {sorted(DEFAULT_TUNE)}")
    c = DEFAULT_TUNE[name] if tune is None else float(tune)
    if not (c > 0.0) or not np.isfinite(c):
        raise ValueError(f"the tuning constant must be positive, got {tune!r}")
    return name, c


def robust_weight(loss, c, s, e):
    """(r, rho) per row from residuals ``e`` and per-row scales ``s`` (fp64, the operations and their order of the kernel's
    ``robust_weight``): rows with s == 0 get r = 1, rho = 0."""
    e = np.asarray(e, dtype=np.float64)
    s = np.broadcast_to(np.asarray(s, dtype=np.float64), e.shape)
    r = np.ones_like(e)
    rho = np.zeros_like(e)
    ok = s > 0.0
    if not ok.any():
        return r, rho
    eo, so = e[ok], s[ok]
    cs = c * so
    ae = np.abs(eo)
    u = eo / so
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if loss == "huber":
            inside = ae <= cs
            ro = np.where(inside, 1.0, np.sqrt(cs / np.where(inside, 1.0, ae)))
            rh = np.where(inside, (u * u) * 0.5, c * np.abs(u) - (c * c) * 0.5)
        elif loss == "bisquare":
            inside = ae < cs
            t = eo / cs
            ro = np.where(inside, 1.0 - t * t, 0.0)
            q = u / c
            v = 1.0 - q * q
            c6 = (c * c) / 6.0
            rh = np.where(inside, c6 * (1.0 - (v * v) * v), c6)
        elif loss == "cauchy":
            t = eo / cs
            ro = 1.0 / np.sqrt(1.0 + t * t)
            q = u / c
            rh = ((c * c) * 0.5) * np.log(1.0 + q * q)
        else:
            raise ValueError(f"unknown loss {loss!r}")
    r[ok] = ro
    rho[ok] = rh
    return r, rho


def class_scales(e, cat, ncat, part):
    """(s, n) per class over the participating rows: s = 1.4826 numpy-median of |e| (0 for an empty class)."""
    s, n = np.zeros(ncat), np.zeros(ncat, dtype=np.int64)
    ae = np.abs(e)
    for g in range(ncat):
        sel = part & (cat == g)
        n[g] = int(np.count_nonzero(sel))
        if n[g]:
            s[g] = MAD_TO_SIGMA * np.median(ae[sel])
    return s, n


def class_table(e, r, rho, cat, ncat, part):
    """The per-class table (ncat x 6) of one iteration: n, rows with omega < 1, rows with omega = 0, sum omega, sum e^2,
    sum rho."""
    out = np.zeros((ncat, 6))
    for g in range(ncat):
        sel = part & (cat == g)
        rg = r[sel]
        out[g] = (rg.size, np.count_nonzero(rg < 1.0), np.count_nonzero(rg == 0.0), np.sum(rg * rg), np.sum(e[sel] ** 2),
                  np.sum(rho[sel]))
    return out


def _ridge_solve(X, y, alpha):
    """argmin |X beta - y|^2 + alpha |beta|^2 through the Jacobi-scaled normal equations (the form of the GPU's solve)."""
    G = X.T @ X
    G[np.diag_indices_from(G)] += alpha
    c = X.T @ y
    d = np.sqrt(np.diag(G))
    d[d == 0.0] = 1.0
    return np.linalg.solve(G / d[:, None] / d[None, :], c / d) / d


class RobustHost(NamedTuple):
    fit: np.ndarray
    iterations: int
    converged: bool
    scales: np.ndarray        # iterations x ncat
    tables: np.ndarray        # iterations x ncat x 6
    omega: np.ndarray         # per row, 1 on rows that do not take part
    start: np.ndarray


def robust_host(A, b, w, mask=None, cat=None, loss="huber", tune=None, alpha=1e-8, ncat=None, scale=None, scale_iters=0,
                max_iter=50, tol=1e-8, start=None):
    """The yardstick: the iteration of the module docstring in numpy fp64 on rows ``A`` (m x K), truths ``b``, base weights
    ``w`` (one per row), training ``mask`` (None = all rows train) and class ids ``cat`` (None = one class).  ``scale``: a
    fixed scale per class instead of the MAD.  Returns ``RobustHost``."""
    A = np.asarray(A, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64).reshape(-1)
    w = np.asarray(w, dtype=np.float64).reshape(-1)
    m = A.shape[0]
    mask = np.ones(m, dtype=bool) if mask is None else np.asarray(mask).astype(bool)
    cat = np.zeros(m, dtype=np.int64) if cat is None else np.asarray(cat, dtype=np.int64)
    ncat = int(ncat) if ncat is not None else (int(cat.max()) + 1 if m else 1)
    loss, c = resolve_loss(loss, tune)
    part = mask & (w > 0.0)
    Ap, bp, wp, cp = A[part], b[part], w[part], cat[part]
    allp = np.ones(len(bp), dtype=bool)
    fixed = None if scale is None else np.asarray(scale, dtype=np.float64).reshape(ncat)
    beta = _ridge_solve(Ap * wp[:, None], bp * wp, alpha) if start is None else np.asarray(start, dtype=np.float64).copy()
    beta0 = beta.copy()
    scales, tables = [], []
    s = np.zeros(ncat) if fixed is None else fixed
    converged, it = False, 0
    r = np.ones(len(bp))
    for t in range(int(max_iter)):
        e = wp * (bp - Ap @ beta)
        if fixed is None and (scale_iters == 0 or t < scale_iters):
            s, _ = class_scales(e, cp, ncat, allp)
        r, rho = robust_weight(loss, c, s[cp], e)
        scales.append(np.array(s, dtype=np.float64))
        tables.append(class_table(e, r, rho, cp, ncat, allp))
        wr = wp * r
        new = _ridge_solve(Ap * wr[:, None], bp * wr, alpha)
        it = t + 1
        done = np.max(np.abs(new - beta)) <= tol * np.max(np.abs(new))
        beta = new
        if done:
            converged = True
            break
    omega = np.ones(m)
    omega[part] = r * r
    return RobustHost(beta, it, converged, np.array(scales).reshape(it, ncat), np.array(tables).reshape(it, ncat, 6), omega,
                      beta0)


class RobustResult:
    """What ``robust_fit`` returns: ``fit`` (on every rank), ``iterations``, ``converged``, ``scales`` (iterations x ncat),
    ``tables`` (iterations x ncat x 6, columns ``TABLE_COLUMNS``, summed over the ranks), ``classes`` (the key of every class
    id), ``loss``, ``tune``, ``start`` (beta_0); ``omega()`` and ``table()`` fetch the per-row diagnostics on first use."""

    def __init__(self, fit, iterations, converged, scales, tables, classes, loss, tune, start, ctx, m, part, labels):
        self.fit, self.iterations, self.converged = fit, iterations, converged
        self.scales, self.tables, self.classes = scales, tables, classes
        self.loss, self.tune, self.start = loss, tune, start
        self._ctx, self._m, self._part, self._labels = ctx, m, part, labels
        self._omega = None

    def omega(self):
        """omega_i = r_i^2 of the last re-weighting for this rank's rows (1 on rows that take no part), downloaded from the
        device on first use -- before the rows of the context change."""
        if self._omega is None:
            if self._m == 0:
                self._omega = np.zeros(0)
            else:
                r = self._ctx.robust_download(e=False, r=True)["r"]
                self._omega = r * r
        return self._omega

    def table(self, by="Configs", fs_dict=None):
        """The suspect units: a DataFrame with one row per ``fs_dict[by]`` label (``by``: "Configs" or "Groups"; ``fs_dict``
        None = the labels of the fit) over this rank's participating rows -- ``count``, ``mean_omega``, ``rejected`` (rows
        with omega = 0), ``downweighted`` (rows with omega < 1) -- sorted by ``mean_omega``, most suspect first."""
        from pandas import DataFrame

        labels = self._labels if fs_dict is None else fs_dict
        if labels is None or by not in labels:
            raise KeyError(f"robust table: no '{by}' labels")
        om = self.omega()
        keys = np.asarray(labels[by], dtype=object)
        if keys.shape[0] != self._m:
            raise ValueError(f"robust table: {keys.shape[0]} labels for {self._m} rows")
        rows = np.flatnonzero(self._part)
        units, inv = np.unique(keys[rows].astype(str), return_inverse=True)
        count = np.bincount(inv, minlength=len(units))
        so = np.bincount(inv, weights=om[rows], minlength=len(units))
        rej = np.bincount(inv, weights=(om[rows] == 0.0), minlength=len(units))
        dwn = np.bincount(inv, weights=(om[rows] < 1.0), minlength=len(units))
        df = DataFrame({by: units, "count": count, "mean_omega": so / np.maximum(count, 1), "rejected": rej.astype(np.int64),
                        "downweighted": dwn.astype(np.int64)})
        return df.sort_values(["mean_omega", by], kind="stable").reset_index(drop=True)


def _classes(solver, by, labels, m):
    """(class id per row int32, keys of the classes) from ``by``: "Row_Type", "Groups+Row_Type", None or an integer array;
    the keys are those of all ranks, sorted."""
    pt = solver.pt
    if by is None:
        return None, [None]
    if isinstance(by, str):
        name = by.strip().lower()
        if name in ("row_type", "groups+row_type"):
            if labels is None or "Row_Type" not in labels or (name != "row_type" and "Groups" not in labels):
                raise KeyError(f"robust_fit: no labels for by={by!r}")
            rt = labels["Row_Type"]
            local = [(str(g), str(r)) for g, r in zip(labels["Groups"], rt)] if name != "row_type" else [str(r) for r in rt]
        elif name in ("none", "global"):
            return None, [None]
        else:
            raise ValueError(f"robust_fit: by={by!r}: one of 'Row_Type', 'Groups+Row_Type', None or an integer array")
        if len(local) != m:
            raise ValueError(f"robust_fit: {len(local)} labels for {m} rows")
        keys = sorted(set(local))
        if pt.multi:
            keys = sorted({k for part in pt.allgather_object(keys) for k in part})
        pos = {k: i for i, k in enumerate(keys)}
        return np.fromiter((pos[k] for k in local), dtype=np.int32, count=m), keys
    cat = np.asarray(by)
    if cat.shape != (m,) or not np.issubdtype(cat.dtype, np.integer):
        raise ValueError(f"robust_fit: an explicit class array needs {m} integers")
    top = int(cat.max()) + 1 if m else 1
    if m and int(cat.min()) < 0:
        raise ValueError("robust_fit: class ids must not be negative")
    if pt.multi:
        top = max(pt.allgather_object(top))
    return cat.astype(np.int32), list(range(top))


def robust_fit(solver, loss="huber", tune=None, alpha=None, by="Row_Type", scale=None, scale_iters=0, max_iter=50, tol=1e-8,
               start=None, a=None, b=None, w=None, fs_dict=None, trainall=False):
    """``Solver.robust_fit``: see there."""
    pt = solver.pt
    if pt.multi and pt.comm_kind != "rccl":
        raise NotImplementedError("robust_fit: the IRLS step runs on the native transports (RCCL / peer-to-peer) only; under a "
                                  "torch.distributed group fit each rank's rows on one GPU, or start the job with comm='rccl'")
    loss, c = resolve_loss(loss, tune)
    if alpha is None:
        sec = solver.config.sections.get("ROBUST") if hasattr(solver.config, "sections") else None
        alpha = sec.alpha if sec is not None else 1e-8
    alpha = float(alpha)
    max_iter, scale_iters, tol = int(max_iter), int(scale_iters), float(tol)
    if max_iter < 1 or scale_iters < 0 or not (tol >= 0.0) or not (alpha >= 0.0):
        raise ValueError("robust_fit: max_iter >= 1, scale_iters >= 0, tol >= 0 and alpha >= 0 are needed")
    a_, b_, w_full, mask, shared_mode = solver._resolve_inputs(a, b, w, fs_dict, trainall)
    if np.ndim(a_) != 2:
        raise ValueError("the A matrix must be 2-D")
    m, K = a_.shape
    if fs_dict is not None:
        labels = fs_dict
    elif a is None:
        labels = pt.local_lists if (pt.multi and getattr(pt, "local_lists", None)) else pt.fitsnap_dict
    else:
        labels = None
    cat, keys = _classes(solver, by, labels, m)
    ncat = len(keys)
    if ncat > _capi.ROBUST_MAX_CLASSES:
        raise ValueError(f"robust_fit: {ncat} classes, the kernels hold {_capi.ROBUST_MAX_CLASSES}: choose a coarser `by`")
    if scale is not None:
        scale = np.asarray(scale, dtype=np.float64).reshape(-1)
        if scale.shape != (ncat,) or not np.all(scale >= 0.0):
            raise ValueError(f"robust_fit: scale needs {ncat} non-negative entries (classes {keys})")
    if start is not None:
        start = np.asarray(start, dtype=np.float64).reshape(-1)
        if start.shape != (K,):
            raise ValueError(f"robust_fit: start has {start.size} entries, the rows have {K} columns")
    have_rows = m > 0
    if not have_rows and not pt.multi:
        raise ValueError("robust_fit: no rows")
    ctx = pt.hip()
    if have_rows:
        ctx = solver._upload(a_, b_, shared_mode)
        solver._push_weights(ctx, w_full, mask)
    elif ctx.m > 0:
        ctx.drop_rows()                 # rows of an EARLIER fit must not stand in for this rank's empty share
        solver._resident_key = None
    solver._stats_host = None
    solver._stats_dev = None

    def fit():
        if pt.multi:
            beta, rank, rcond, ptr = ctx.fit_dist(_capi.SOLVE_RIDGE, alpha, K)      # collective
        else:
            beta, rank, rcond, ptr = ctx.fit_resident(_capi.SOLVE_RIDGE, alpha)
        solver._stats_dev = (ctx, ptr, K)
        solver.last_rank, solver.last_rcond = rank, rcond
        return beta

    beta = fit() if start is None else start.copy()
    beta0 = beta.copy()
    scales, tables = [], []
    converged, it = False, 0
    s = scale
    ctx.robust_begin(cat, ncat)
    try:
        for t in range(max_iter):
            if scale is None and (scale_iters == 0 or t < scale_iters):
                ctx.robust_residuals(beta)
                s, _ = ctx.robust_scale()                                           # collective
                sums = ctx.robust_reweight(loss, c)
            else:
                # the scales are known: residuals and weights in one launch (a fixed scale is sent once)
                sums = ctx.robust_step(beta, loss, c, scale=s if t == 0 else None)
            if pt.multi:
                pt.allreduce_host(sums)
            scales.append(np.array(s, dtype=np.float64))
            tables.append(sums)
            new = fit()
            it = t + 1
            done = np.max(np.abs(new - beta)) <= tol * np.max(np.abs(new))
            beta = new
            if done:
                converged = True
                break
    finally:
        ctx.robust_end()                # the context's weights and mask are those of the caller again
        solver._stats_dev = None        # (the statistics left on the device are those of the last w r, not of a plain fit)
    mask_b = np.asarray(mask).astype(bool)
    wf = w_full.full() if hasattr(w_full, "full") else np.asarray(w_full, dtype=np.float64)
    part = mask_b & (wf > 0.0) if have_rows else np.zeros(0, dtype=bool)
    if pt._rank == 0:
        solver.fit = beta
    return RobustResult(beta, it, converged, np.array(scales).reshape(it, ncat), np.array(tables).reshape(it, ncat, 6), keys,
                        loss, c, beta0, ctx, m, part, labels)


class ROBUST(Solver):
    """Plugin solver ``[SOLVER] solver = ROBUST``: ``perform_fit`` runs ``robust_fit`` with the ``[ROBUST]`` section (``loss``,
    ``tune``, ``alpha``, ``scale_by`` = row_type / groups+row_type / none, ``scale_iters``, ``max_iter``, ``tol``) and leaves
    the result object in ``self.robust``; ``error_analysis`` afterwards reads the base weights, as after any linear fit."""

    SCALE_BY = {"row_type": "Row_Type", "groups+row_type": "Groups+Row_Type", "none": None, "global": None}

    def __init__(self, name, pt, config):
        super().__init__(name, pt, config)
        self.robust = None

    def perform_fit(self, a=None, b=None, w=None, fs_dict=None, trainall=False):
        """Same call contract as ``RIDGE.perform_fit``; explicit arrays without ``fs_dict`` carry no row labels, so they
        are fitted with one global scale unless ``scale_by = none`` already says so."""
        sec = self.config.sections["ROBUST"]
        if sec.scale_by not in self.SCALE_BY:
            raise ValueError(f"[ROBUST] scale_by = {sec.scale_by!r}: one of {sorted(self.SCALE_BY)}")
        by = self.SCALE_BY[sec.scale_by]
        if a is not None and (fs_dict is None or "Row_Type" not in fs_dict):
            by = None
        self.robust = robust_fit(self, loss=sec.loss, tune=sec.tune, alpha=sec.alpha, by=by, scale_iters=sec.scale_iters,
                                 max_iter=sec.max_iter, tol=sec.tol, a=a, b=b, w=w, fs_dict=fs_dict, trainall=trainall)
