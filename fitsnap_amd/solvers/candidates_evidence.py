"""Marginal likelihood (evidence) of the group-weight candidates of ``CandidateFits`` and its gradient over the scales
(``CandidateFits.evidence``, ``CandidateFits.maximise_evidence``).

The weights are read as inverse noise standard deviations: candidate p gives the rows of category c the weights
w_r = w0_r S[p, c], lambda_c = S[p, c]^2.  A category is ACTIVE when it is a training category, S[p, c] != 0 and it has n_c > 0
rows with w0 != 0; N = sum of n_c over the active categories.  With the packed blocks [G_c | r_c | bb_c, ., .] of
``fsnap_cat_normal_eq`` and a column called dead when sum_c lambda_c G_c,jj = 0 (beta_j = 0, left out of everything):

    S = sum_active lambda_c G_c + alpha I,   q = sum_active lambda_c r_c          (live columns, k of them)
    beta = S^-1 q,   Q_c = bb_c - 2 beta . r_c + beta' G_c beta,   T_c = tr(S^-1 G_c),   gamma_c = lambda_c T_c
    R = sum_active lambda_c Q_c + alpha |beta|^2,   N' = N (alpha > 0) or N - k (alpha = 0)

    scale="fixed"     L = sum log|w_r| + (k / 2) log alpha - 1/2 log|S| - R / 2 - (N' / 2) log 2 pi
    scale="profiled"  sigma^2 = R / N',  L = sum log|w_r| + (k / 2) log alpha - 1/2 log|S| - (N' / 2) (log sigma^2 + 1 + log 2 pi)

(the (k / 2) log alpha term is absent at alpha = 0: the restricted likelihood of a variance-components model; with a ridge term
it is MacKay's evidence, the prior being beta ~ N(0, 1 / alpha) or N(0, sigma^2 / alpha)).  With kappa = 1 (fixed) or
1 / sigma^2 (profiled):

    dL/dlog S[p, c] = n_c - gamma_c - kappa lambda_c Q_c   (active c; 0 otherwise)
    dL/dlog alpha   = (k - alpha tr(S^-1) - kappa alpha |beta|^2) / 2          (0 at alpha = 0)

Invariants: sum_c gamma_c + alpha tr(S^-1) = k; sum_c dL/dlog S + 2 dL/dlog alpha = 0 (profiled) or N' - R (fixed).

The device route (``fsnap_candidates_evidence``, kernels E1-E3 of csrc/fsnap_evidence.hip, K <= 144) returns beta, log|S|,
tr(S^-1) and the two inner products T_c, Q_c of every block; ``assemble`` turns them into the table above in float64 numpy.
``host_evidence`` is the same from downloaded blocks in plain numpy: the check, the baseline and the route beyond 144 columns.
"""
from __future__ import annotations

import numpy as np

from .. import _capi
from . import candidates_cv

MAX_K = candidates_cv.MAX_K
METHODS = ("auto", "device", "host")
SCALES = ("profiled", "fixed")
PIVOT_TOL = 1e-10            # fsnap::LOCO_PIVOT_TOL (loco.PIVOT_TOL)
LOG_2PI = float(np.log(2.0 * np.pi))
FIELDS = ("log_evidence", "beta", "logdet", "sigma2", "rss", "dof", "noise", "grad_logS", "grad_logalpha", "live", "status",
          "min_pivot")


def choose_method(method, K):
    """"device" or "host" for K columns; ValueError for an unknown method or method="device" beyond K = 144."""
    if method not in METHODS:
        raise ValueError(f"evidence: method must be one of {', '.join(METHODS)}")
    if method == "device" and K > MAX_K:
        raise ValueError(f"evidence: method='device' needs K <= {MAX_K} (K = {K})")
    if method == "auto":
        return "device" if K <= MAX_K else "host"
    return method


def check_scale(scale):
    if scale not in SCALES:
        raise ValueError(f"evidence: scale must be one of {', '.join(SCALES)}")
    return scale


def check_alpha(alpha):
    alpha = float(alpha)
    if not np.isfinite(alpha) or alpha < 0.0:
        raise ValueError(f"evidence: alpha = {alpha} is negative or not finite")
    return alpha


def active_mask(S, training, n):
    """(P, C) bool: training category, S != 0 and n_c > 0."""
    return (np.asarray(S) != 0) & (np.asarray(training, dtype=bool) & (np.asarray(n) > 0))[None, :]


class CandidateEvidence:
    """Result of ``CandidateFits.evidence`` for P candidates, C categories, K columns.

    ``log_evidence`` (P,): L; ``beta`` (P, K); ``logdet`` (P,): log|S|; ``sigma2`` (P,): the profiled common noise scale (1 under
    ``scale="fixed"``); ``rss`` (P, C): Q_c; ``dof`` (P, C): gamma_c, the effective number of parameters category c determines;
    ``noise`` (P, C): Q_c / (n_c - gamma_c), the noise variance of the category in units of 1 / w0^2 (NaN where the denominator
    is <= 0 or c is inactive); ``grad_logS`` (P, C): dL/dlog|S|; ``grad_logalpha`` (P,): dL/dlog alpha; ``live`` (P,): k;
    ``status`` (P,): 0, or 1 where a scaled pivot was not above 1e-10 -- every field of that candidate is NaN; ``min_pivot``
    (P,): the smallest scaled pivot met; ``active`` (P, C) bool; ``method``; ``scale``; ``alpha``."""

    def __init__(self, **fields):
        for name, value in fields.items():
            setattr(self, name, value)


def assemble(S, alpha, scale, active, n, slw0, beta, logdet, trinv, live, status, min_pivot, T, Q, method="host"):
    """The table of a ``CandidateEvidence`` in float64 numpy from the per-candidate solves (beta (P, K), log|S|, tr(S^-1), live
    columns, status, smallest pivot) and the two inner products of every block, T (P, C) = tr(S^-1 G_c) and Q (P, C) =
    bb_c - 2 beta . r_c + beta' G_c beta.  ``n`` (C,): rows with w0 != 0 per category, ``slw0`` (C,): their sum of log|w0|.  The
    sums over the categories run in index order."""
    S = np.asarray(S, dtype=np.float64)
    P, C = S.shape
    active = np.asarray(active, dtype=bool)
    n = np.asarray(n, dtype=np.float64)
    lam = np.where(active, S * S, 0.0)
    Q = np.where(active, np.asarray(Q, dtype=np.float64), 0.0)
    gamma = lam * np.where(active, np.asarray(T, dtype=np.float64), 0.0)
    k = np.asarray(live, dtype=np.float64)
    bb = np.einsum("pk,pk->p", beta, beta)
    N = np.zeros(P)
    R = np.zeros(P)
    slw = np.zeros(P)
    with np.errstate(divide="ignore", invalid="ignore"):
        logS = np.where(active, np.log(np.abs(np.where(active, S, 1.0))), 0.0)
        for c in range(C):
            N = N + np.where(active[:, c], n[c], 0.0)
            R = R + lam[:, c] * Q[:, c]
            slw = slw + np.where(active[:, c], slw0[c] + n[c] * logS[:, c], 0.0)
        R = R + alpha * bb
        Np = N if alpha > 0 else N - k
        head = slw - 0.5 * logdet + (0.5 * k * np.log(alpha) if alpha > 0 else 0.0)
        if scale == "fixed":
            sigma2 = np.ones(P)
            kappa = np.ones(P)
            L = head - 0.5 * R - 0.5 * Np * LOG_2PI
        else:
            sigma2 = np.where((Np > 0) & (R > 0), R / Np, np.nan)
            kappa = 1.0 / sigma2
            L = head - 0.5 * Np * (np.log(sigma2) + 1.0 + LOG_2PI)
        grad = np.where(active, n[None, :] - gamma - kappa[:, None] * lam * Q, 0.0)
        gla = 0.5 * (k - alpha * trinv - kappa * alpha * bb) if alpha > 0 else np.zeros(P)
        den = n[None, :] - gamma
        noise = np.where(active & (den > 0), Q / np.where(den > 0, den, 1.0), np.nan)
    out = dict(log_evidence=L, beta=np.array(beta, dtype=np.float64), logdet=np.array(logdet, dtype=np.float64), sigma2=sigma2,
               rss=Q, dof=gamma, noise=noise, grad_logS=grad, grad_logalpha=gla, live=k.copy(),
               status=np.asarray(status, dtype=np.int64).copy(), min_pivot=np.array(min_pivot, dtype=np.float64))
    bad = out["status"] != 0
    for name in FIELDS:
        if name not in ("status", "min_pivot"):
            out[name] = np.array(out[name], dtype=np.float64)
            out[name][bad] = np.nan
    return CandidateEvidence(active=active, method=method, scale=scale, alpha=float(alpha), **out)


def host_solves(blocks, S, alpha, active, K):
    """The per-candidate part in numpy float64 from the C packed blocks: (beta (P, K), log|S| (P,), tr(S^-1) (P,), live (P,),
    status (P,), smallest scaled pivot (P,), T (P, C), Q (P, C)).  The live rule, the Jacobi scaling and the pivot rule are the
    device's; the inverse is formed explicitly from the Cholesky factor."""
    blocks = np.asarray(blocks, dtype=np.float64)
    S = np.asarray(S, dtype=np.float64)
    P, C = S.shape
    KK = K * K
    G, r, bb = blocks[:, :KK].reshape(C, K, K), blocks[:, KK:KK + K], blocks[:, KK + K]
    gdiag = np.einsum("ckk->ck", G)
    beta = np.zeros((P, K))
    logdet, trinv, live_n, status = np.zeros(P), np.zeros(P), np.zeros(P), np.zeros(P, dtype=np.int64)
    minpiv = np.full(P, np.inf)
    T, Q = np.zeros((P, C)), np.zeros((P, C))
    for p in range(P):
        lam = np.where(active[p], S[p] * S[p], 0.0)
        live = (lam @ gdiag) != 0.0
        k = int(live.sum())
        live_n[p] = k
        Sinv = np.zeros((K, K))
        if k:
            H = np.tensordot(lam, G, axes=1)[np.ix_(live, live)] + alpha * np.eye(k)
            d = np.sqrt(np.diag(H))
            try:
                Lf = np.linalg.cholesky(H / d[:, None] / d[None, :])
                minpiv[p] = float(np.min(np.diag(Lf)) ** 2)
            except np.linalg.LinAlgError:
                minpiv[p], status[p] = 0.0, 1
            if status[p] == 0 and not minpiv[p] > PIVOT_TOL:
                status[p] = 1
            if status[p]:
                continue
            Li = np.linalg.solve(Lf, np.eye(k))
            q = (lam @ r)[live]
            beta[p, live] = (Li.T @ (Li @ (q / d))) / d
            Sinv[np.ix_(live, live)] = (Li.T @ Li) / d[:, None] / d[None, :]
            logdet[p] = 2.0 * float(np.sum(np.log(np.diag(Lf)) + np.log(d)))
            trinv[p] = float(np.trace(Sinv))
        T[p] = np.einsum("ij,cij->c", Sinv, G)
        Q[p] = bb - 2.0 * (r @ beta[p]) + np.einsum("i,cij,j->c", beta[p], G, beta[p])
    return beta, logdet, trinv, live_n, status, minpiv, T, Q


def host_evidence(blocks, S, alpha, n, slw0, training, K, scale="profiled"):
    """``CandidateFits.evidence`` in plain numpy from the C packed blocks (C x (K^2 + K + 3)); ``n`` / ``slw0`` (C,): the rows
    with w0 != 0 per category and their sum of log|w0|; ``training`` (C,) bool.  Needs no GPU."""
    check_scale(scale)
    alpha = check_alpha(alpha)
    S = np.asarray(S, dtype=np.float64)
    active = active_mask(S, training, n)
    parts = host_solves(blocks, S, alpha, active, K)
    return assemble(S, alpha, scale, active, n, slw0, *parts, method="host")


def evidence_constants(cf):
    """(n (C,), sum log|w0| (C,), training (C,)) of a ``CandidateFits``: the rows with w0 != 0 per category over all ranks."""
    held = getattr(cf, "_evidence_const", None)
    if held is None:
        keep = (cf.cat >= 0) & (cf.w0 != 0)
        cat = cf.cat[keep].astype(np.int64)
        both = np.zeros(2 * cf.ncat)
        both[:cf.ncat] = np.bincount(cat, minlength=cf.ncat)
        both[cf.ncat:] = np.bincount(cat, weights=np.log(np.abs(cf.w0[keep])), minlength=cf.ncat)
        if cf.pt.multi:
            cf.pt.allreduce_host(both)
        held = cf._evidence_const = (both[:cf.ncat].copy(), both[cf.ncat:].copy(), np.array([not k[1] for k in cf.keys], dtype=bool))
    return held


def default_alpha(cf, alpha):
    if alpha is not None:
        return check_alpha(alpha)
    kind, param, _ = cf._kind()
    return float(param) if kind in (_capi.SOLVE_RIDGE, _capi.SOLVE_RIDGE_INV) else 0.0


def evidence(cf, S, alpha=None, scale="profiled", method="auto"):
    """``CandidateFits.evidence``: see there."""
    from .candidates import check_scales
    from .candidates_cv_grad import download_blocks

    check_scale(scale)
    S = check_scales(S, cf.ncat)
    method = choose_method(method, cf.K)
    alpha = default_alpha(cf, alpha)
    ctx = cf._device()
    n, slw0, training = evidence_constants(cf)
    active = active_mask(S, training, n)
    if method == "device":
        beta, info, Y = ctx.candidates_evidence(cf._layout, alpha, S, active, cf.K)
        parts = (beta, info[:, 3], info[:, 4], info[:, 2], info[:, 0].astype(np.int64), info[:, 1], Y[:, :, 0], Y[:, :, 1])
    else:
        parts = host_solves(download_blocks(ctx, cf._stats, cf.ncat, cf.K), S, alpha, active, cf.K)
    return assemble(S, alpha, scale, active, n, slw0, *parts, method=method)


def fixed_point(evaluate, S0, n, steps=50, tol=1e-6, damping=1.0, max_halvings=8):
    """Batched safeguarded fixed-point ascent of L on theta = log|S| from the P starts S0; ``evaluate(S)`` -> CandidateEvidence.
    The step is theta_c += eta / 2 log((n_c - gamma_c) / (kappa lambda_c Q_c)) on the active categories whose numerator and
    denominator are positive; a candidate accepts a trial only if its L does not decrease, otherwise its eta is halved (at most
    ``max_halvings`` times per iteration); after an accepted step eta doubles, up to ``damping``.  Returns (S, evidence at S,
    history (iterations + 1, P) of the accepted L, converged (P,))."""
    S = np.array(S0, dtype=np.float64)
    if steps < 0 or not tol > 0 or not 0 < damping <= 1:
        raise ValueError("maximise_evidence: needs steps >= 0, tol > 0 and 0 < damping <= 1")
    P = S.shape[0]
    n = np.asarray(n, dtype=np.float64)
    eta = np.full(P, float(damping))
    ev = evaluate(S)
    history = [np.array(ev.log_evidence)]

    def done(e):
        with np.errstate(invalid="ignore", divide="ignore"):
            rel = np.where(e.active, np.abs(e.grad_logS) / np.where(n > 0, n, 1.0)[None, :], 0.0)
            return np.max(rel, axis=1) <= tol               # NaN compares false: a failed candidate never converges

    converged = done(ev)
    for _ in range(steps):
        alive = np.isfinite(ev.log_evidence) & ~converged
        if not alive.any():
            break
        with np.errstate(invalid="ignore", divide="ignore"):
            kappa = 1.0 / ev.sigma2
            num = n[None, :] - ev.dof
            den = kappa[:, None] * (S * S) * ev.rss
            ok = ev.active & (num > 0) & (den > 0) & alive[:, None]
            step = np.where(ok, 0.5 * np.log(np.where(ok, num, 1.0) / np.where(ok, den, 1.0)), 0.0)
        pending = alive & (step != 0).any(axis=1)
        L = np.array(ev.log_evidence)
        for _ in range(max_halvings + 1):
            if not pending.any():
                break
            trial = np.where(pending[:, None], S * np.exp(eta[:, None] * step), S)
            tv = evaluate(trial)
            with np.errstate(invalid="ignore"):
                accept = pending & (tv.log_evidence >= L)   # a NaN trial is never accepted
            S[accept] = trial[accept]
            L[accept] = tv.log_evidence[accept]
            eta[accept] = np.minimum(2.0 * eta[accept], damping)
            pending &= ~accept
            eta[pending] *= 0.5
        ev = evaluate(S)
        history.append(np.array(ev.log_evidence))
        converged = done(ev)
    return S, ev, np.array(history), converged


def maximise_evidence(cf, S0, alpha=None, scale="profiled", steps=50, tol=1e-6, damping=1.0, method="auto"):
    """``CandidateFits.maximise_evidence``: see there."""
    from .candidates import check_scales

    check_scale(scale)
    S0 = check_scales(S0, cf.ncat)
    choose_method(method, cf.K)
    alpha = default_alpha(cf, alpha)
    n = evidence_constants(cf)[0]
    return fixed_point(lambda S: evidence(cf, S, alpha, scale, method), S0, n, steps, tol, damping)
