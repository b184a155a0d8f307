"""Gradient of the cross-validated cost of ``CandidateFits`` over the group weights, and a plain batched descent on it
(``CandidateFits.cross_validate_gradient``, ``CandidateFits.descend_weights``).

The objective is taken on the BASE-weighted held-out residuals -- entry 3 of the four sums of ``fsnap_cv_candidate_rows``,
sum (w0 r)^2 per composite category, before any scaling by S:

    E[p, t] = sum over the training categories c of row type t, the folds f and the rows i of (f, c) of (w0_i (t_i - a_i beta[p, f]))^2
    n_t     = the number of those rows
    J[p]    = sum_t wt[t] phi(E[p, t] / n_t),      phi = sqrt ("rmse") or the identity ("mse")

With w0 = 1 on the training rows this is ``CandidateCV.cost(weights, "rmse")`` exactly.  The S-scaled sums (``w_rmse``) are not
used: they go to 0 with S, so a descent on them would switch every category off instead of fitting the held-out rows.

The chain rule gives per-category coefficients omega[p, c] = wt[t(c)] phi'(E[p, t] / n_t) / n_t (0 for testing categories, for row
types of weight 0 and where n_t = 0), and the adjoint of the K x K solve of problem (p, f) -- on its live columns, the live set
treated as fixed -- gives, with B[f, c] the blocks and R[f, c] = T[c] - B[f, c],

    g[p, f]      = 2 sum_c omega[p, c] (B[f, c].G beta[p, f] - B[f, c].r)
    lambda[p, f] = H^-1 g[p, f],              H = sum_c S[p, c]^2 R[f, c].G + alpha I
    D[p, f, c]   = lambda[p, f] . (R[f, c].r - R[f, c].G beta[p, f])
    dJ/dS[p, c]  = 2 S[p, c] sum_f D[p, f, c],    dJ/dlog S = S dJ/dS,    dJ/dlog alpha[p] = -alpha sum_f lambda[p, f] . beta[p, f]

so all C partial derivatives of a candidate cost one more solve per fold and two sweeps over the blocks
(``fsnap_cv_candidates_grad``, csrc/fsnap_cvgrad.hip, K <= 144).  Scaling every S[p, .]^2 and alpha by one factor changes no
beta: sum_c dJ/dlog S[p, c] = -2 dJ/dlog alpha[p].  ``host_gradient`` is the same in plain numpy from downloaded blocks.
"""
from __future__ import annotations

import numpy as np

from .. import _capi
from . import candidates_cv

MAX_K = candidates_cv.MAX_K
METHODS = ("auto", "device", "host")
METRICS = ("rmse", "mse")
PIVOT_TOL = 1e-10            # fsnap::LOCO_PIVOT_TOL


def choose_method(method, K):
    """"device" or "host" for K columns; ValueError for an unknown method or method="device" beyond K = 144."""
    if method not in METHODS:
        raise ValueError(f"cross_validate_gradient: method must be one of {', '.join(METHODS)}")
    if method == "device" and K > MAX_K:
        raise ValueError(f"cross_validate_gradient: method='device' needs K <= {MAX_K} (K = {K})")
    if method == "auto":
        return "device" if K <= MAX_K else "host"
    return method


def type_weights(weights, row_types):
    """One weight per entry of ``row_types`` from a mapping row type -> weight (missing types count 0) or a sequence."""
    if hasattr(weights, "keys"):
        unknown = [t for t in weights if t not in row_types]
        if unknown:
            raise ValueError(f"cross_validate_gradient: no rows of type {unknown[0]!r} (row types: {row_types})")
        return np.array([float(weights.get(t, 0.0)) for t in row_types])
    wt = np.asarray(weights, dtype=np.float64).reshape(-1)
    if wt.shape[0] != len(row_types):
        raise ValueError(f"cross_validate_gradient: {wt.shape[0]} weights for the row types {row_types}")
    return wt


def objective(base_sums, keys, weights, metric="rmse"):
    """(J (P,), omega (P, C), row types) from the base-weighted pooled sums (P, C, 5: n, sum|r|, sum r^2, sum|w0 r|, sum (w0 r)^2
    of the held-out rows per category of ``keys``, no scaling by S).  The categories of a row type are added in ``keys`` order and
    the types in sorted order, as ``CandidateCV.cost`` adds them.  omega is 0 for testing categories, for types of weight 0,
    where n_t = 0 and (metric "rmse") where E[p, t] = 0, the kink of the square root."""
    if metric not in METRICS:
        raise ValueError(f"cross_validate_gradient: metric must be one of {', '.join(METRICS)}")
    base_sums = np.asarray(base_sums, dtype=np.float64)
    P, C = base_sums.shape[:2]
    row_types = sorted({k[2] for k in keys})
    wt = type_weights(weights, row_types)
    E = np.zeros((P, len(row_types)))
    n = np.zeros(len(row_types))
    tof = np.full(C, -1)
    for c, k in enumerate(keys):
        if not k[1]:
            t = row_types.index(k[2])
            tof[c] = t
            E[:, t] += base_sums[:, c, 4]
            n[t] += base_sums[0, c, 0] if P else 0.0
    J = np.zeros(P)
    omega = np.zeros((P, C))
    for t in range(len(row_types)):
        if wt[t] == 0.0:
            continue
        with np.errstate(divide="ignore", invalid="ignore"):
            mean = E[:, t] / n[t]
            if metric == "rmse":
                val = np.sqrt(mean)
                slope = np.where(mean > 0, 0.5 / val, 0.0) / n[t]
            else:
                val = mean
                slope = np.full(P, 1.0 / n[t])
        J = J + wt[t] * val
        if n[t] > 0:
            slope = np.where(np.isnan(mean), np.nan, slope)
            omega[:, tof == t] = (wt[t] * slope)[:, None]
    return J, omega, row_types


def host_gradient(blocks, S, omega, coef, F, C, K, alpha):
    """``fsnap_cv_candidates_grad`` restated in numpy float64 from the F C packed blocks: (grad_S (P, C), grad_log_alpha (P,),
    lambda (P, F, K), g (P, F, K), info (P, F, 2): status, smallest scaled pivot).  A problem with NaN coefficients or a failed
    Cholesky has status 1 and NaN lambda; its candidate's gradient row is NaN."""
    blocks = np.asarray(blocks, dtype=np.float64).reshape(F, C, -1)
    S = np.asarray(S, dtype=np.float64)
    omega = np.asarray(omega, dtype=np.float64)
    coef = np.asarray(coef, dtype=np.float64)
    P = S.shape[0]
    KK = K * K
    total = blocks[0].copy()
    for f in range(1, F):
        total = total + blocks[f]
    rest = total[None] - blocks
    BG, Br = blocks[:, :, :KK].reshape(F, C, K, K), blocks[:, :, KK:KK + K]
    RG, Rr = rest[:, :, :KK].reshape(F, C, K, K), rest[:, :, KK:KK + K]
    tdiag = np.einsum("ckk->ck", total[:, :KK].reshape(C, K, K))
    grad = np.zeros((P, C))
    gla = np.zeros(P)
    lam = np.zeros((P, F, K))
    g = np.zeros((P, F, K))
    info = np.zeros((P, F, 2))
    for p in range(P):
        s2 = S[p] * S[p]
        om = np.where(np.isfinite(omega[p]), omega[p], 0.0)
        tp = s2 @ tdiag
        for f in range(F):
            beta = coef[p, f]
            g[p, f] = 2.0 * (np.tensordot(om, BG[f], axes=1) @ beta - om @ Br[f])
            Qm = np.tensordot(s2, RG[f], axes=1)
            qjj = np.diag(Qm)
            live = ~((tp == 0.0) | (qjj <= PIVOT_TOL * tp))
            k = int(live.sum())
            status, minpiv = 0, np.inf
            if not np.isfinite(beta).all():
                status = 1
            if k and not status:
                H = Qm[np.ix_(live, live)] + alpha * np.eye(k)
                d = np.sqrt(np.diag(H))
                try:
                    L = np.linalg.cholesky(H / d[:, None] / d[None, :])
                    minpiv = float(np.min(np.diag(L)) ** 2)
                except np.linalg.LinAlgError:
                    minpiv, status = 0.0, 1
                if status == 0 and not minpiv > PIVOT_TOL:
                    status = 1
                if status == 0:
                    y = np.linalg.solve(L, g[p, f, live] / d)
                    lam[p, f, live] = np.linalg.solve(L.T, y) / d
            info[p, f] = (status, minpiv)
            if status:
                lam[p, f] = np.nan
                grad[p] = np.nan
                gla[p] = np.nan
                continue
            D = (Rr[f] - RG[f] @ beta) @ lam[p, f]
            grad[p] += D
            gla[p] += lam[p, f] @ beta
        grad[p] *= 2.0 * S[p]
        gla[p] *= -alpha
    return grad, gla, lam, g, info


class CandidateCVGradient:
    """Result of ``CandidateFits.cross_validate_gradient``.

    ``cv``: the ``CandidateCV`` of the same call; ``cost`` (P,): J; ``grad_S`` (P, ncat): dJ/dS; ``grad_log`` (P, ncat):
    dJ/dlog|S| = S dJ/dS; ``grad_log_alpha`` (P,): dJ/dlog alpha (0 for SVD, alpha = 0); ``omega`` (P, ncat); ``status`` (P, F):
    0, or 1 where the refit or the adjoint solve failed -- that candidate's cost and gradient row are NaN; ``method``."""

    def __init__(self, cv, cost, grad_S, grad_log, grad_log_alpha, omega, status, method):
        self.cv = cv
        self.cost = cost
        self.grad_S = grad_S
        self.grad_log = grad_log
        self.grad_log_alpha = grad_log_alpha
        self.omega = omega
        self.status = status
        self.method = method


def download_blocks(ctx, ptr, nblocks, K):
    """(nblocks, K^2 + K + 3) packed blocks from device address ``ptr``."""
    T = K * K + K + 3
    out = np.empty((nblocks, T))
    for i in range(nblocks):
        G, c, s = ctx.download_packed(ptr + i * T * 8, K)
        out[i, :K * K] = G.ravel()
        out[i, K * K:K * K + K] = c
        out[i, K * K + K:] = s
    return out


def cross_validate_gradient(cf, S, weights, metric="rmse", folds=5, by="Configs", seed=0, method="auto"):
    """``CandidateFits.cross_validate_gradient``: see there."""
    from .candidates import check_scales

    if metric not in METRICS:
        raise ValueError(f"cross_validate_gradient: metric must be one of {', '.join(METRICS)}")
    S = check_scales(S, cf.ncat)
    K, C = cf.K, cf.ncat
    method = choose_method(method, K)
    type_weights(weights, sorted({k[2] for k in cf.keys}))           # argument errors before any device work
    cv = candidates_cv.cross_validate(cf, S, folds, by, seed, "device" if K <= MAX_K else "composed")
    cost, omega, _ = objective(cv.base_sums, cf.keys, weights, metric)
    failed = np.asarray(cv.status).any(axis=1)
    cost = np.where(failed, np.nan, cost)
    omega[failed] = np.nan
    tag, _, F, ptr = cf._cv
    kind, param, _ = cf._kind()
    alpha = float(param) if kind in (_capi.SOLVE_RIDGE, _capi.SOLVE_RIDGE_INV) else 0.0
    ctx = cf.pt.hip()
    if method == "device":
        # a failed candidate's omega is passed as 0 (the call wants finite entries); its NaN coefficients make its row NaN
        grad_S, gla, _, info = ctx.cv_candidates_grad(tag, alpha, S, np.where(failed[:, None], 0.0, omega), cv.coef)
    else:
        grad_S, gla, _, _, info = host_gradient(download_blocks(ctx, ptr, F * C, K), S, omega, cv.coef, F, C, K, alpha)
    status = np.maximum(np.asarray(cv.status, dtype=np.int64), info[:, :, 0].astype(np.int64))
    bad = status.any(axis=1)
    cost = np.where(bad, np.nan, cost)
    grad_S[bad] = np.nan
    gla = np.where(bad, np.nan, gla)
    return CandidateCVGradient(cv, cost, grad_S, S * grad_S, gla, omega, status, method)


def armijo_descent(evaluate, trial_cost, S0, steps=20, eta0=0.5, c1=1e-4, max_halvings=8):
    """Batched steepest descent on theta = log|S| for all P starts at once.  ``evaluate(S)`` -> (cost (P,), grad_log (P, C));
    ``trial_cost(S)`` -> cost (P,).  Per iteration ONE ``evaluate`` call, then line-search rounds of ONE ``trial_cost`` call over
    the P trial points S exp(-eta grad_log): candidate p accepts when cost <= cost_p - c1 eta_p |grad_log_p|^2 (Armijo),
    otherwise eta_p is halved, at most ``max_halvings`` times (then the candidate stays where it is for this iteration).  After
    an accepted step eta_p doubles.  Entries with S = 0 stay 0 (their log-gradient is 0) and signs are kept.  A candidate with a
    NaN cost or gradient is left alone.  Returns (S, history (steps + 1, P), accepted step sizes (steps, P), 0 = no step)."""
    S = np.array(S0, dtype=np.float64)
    if S.ndim != 2:
        raise ValueError("descend_weights: S0 must be (P, ncat)")
    if steps < 0 or max_halvings < 0 or not eta0 > 0 or not 0 < c1 < 1:
        raise ValueError("descend_weights: needs steps >= 0, max_halvings >= 0, eta0 > 0 and 0 < c1 < 1")
    P = S.shape[0]
    eta = np.full(P, float(eta0))
    history = np.full((steps + 1, P), np.nan)
    taken = np.zeros((steps, P))
    if steps == 0:
        history[0] = np.asarray(trial_cost(S), dtype=np.float64)
    for it in range(steps):
        cost, glog = evaluate(S)
        cost, glog = np.array(cost, dtype=np.float64), np.asarray(glog, dtype=np.float64)
        history[it] = cost
        alive = np.isfinite(cost) & np.isfinite(glog).all(axis=1)
        glog = np.where(alive[:, None], glog, 0.0)
        sq = (glog * glog).sum(axis=1)
        pending = alive & (sq > 0)
        for _ in range(max_halvings + 1):
            if not pending.any():
                break
            trial = np.where(pending[:, None], S * np.exp(-eta[:, None] * glog), S)
            tc = np.asarray(trial_cost(trial), dtype=np.float64)
            with np.errstate(invalid="ignore"):
                accept = pending & (tc <= cost - c1 * eta * sq)         # a NaN trial cost is never accepted
            S[accept] = trial[accept]
            cost[accept] = tc[accept]
            taken[it, accept] = eta[accept]
            eta[accept] *= 2.0
            pending &= ~accept
            eta[pending] *= 0.5                                         # kept for the next iteration when no step is found
        history[it + 1] = cost
    return S, history, taken


def descend_weights(cf, S0, weights, metric="rmse", steps=20, folds=5, by="Configs", seed=0, eta0=0.5, c1=1e-4, max_halvings=8):
    """``CandidateFits.descend_weights``: see there."""
    from .candidates import check_scales

    S0 = check_scales(S0, cf.ncat)

    def evaluate(S):
        r = cross_validate_gradient(cf, S, weights, metric, folds, by, seed, "auto")
        return r.cost, r.grad_log

    def trial_cost(S):
        cv = candidates_cv.cross_validate(cf, S, folds, by, seed, "device" if cf.K <= MAX_K else "composed")
        cost = objective(cv.base_sums, cf.keys, weights, metric)[0]
        return np.where(np.asarray(cv.status).any(axis=1), np.nan, cost)

    return armijo_descent(evaluate, trial_cost, S0, steps, eta0, c1, max_halvings)
