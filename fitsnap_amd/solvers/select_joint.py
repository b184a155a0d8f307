"""Host side of the joint unit scores for active learning (``Solver.unit_scores`` / ``Solver.select_units``; ``fsnap_joint_*``,
csrc/fsnap_joint.hip).

``Solver.select_batch`` ranks units by the sum, max or mean of their rows' MARGINAL variances.  The rows of one configuration
are strongly correlated, so the sum counts the same information many times and the max ignores all rows but one; and a unit
of high own variance may be an outlier that teaches nothing about the configurations one cares about.  For a linear-Gaussian
model both defects have exact, label-free cures.  With the posterior C = M M^T (M: K x J), the noise variance tau of a
unit-weight row, the weighted rows X = diag(omega) A_u (n x K) of unit u and Z = X M:

    gain_u      = 1/2 logdet(I + X C X^T / tau)                    the information the unit's labels carry (joint, not summed)
    reduction_u = tr(T C) - tr(T C'_u),  C'_u = tau (P + X^T X)^+  the drop of the total predictive variance over a TARGET set
                                                                   with Gram T = sum_j s_j t_j t_j^T (integrated variance, ALC)

Both come from one small Cholesky per unit, S = I + Z Z^T / tau (n <= J, "n space") or I + Z^T Z / tau (n > J, "J space")
= L L^T -- the same value in either space (Sylvester):

    gain = sum log L_ii
    reduction = ||L^-1 Z B||_F^2 / tau  (n space)  =  ||B||_F^2 - ||L^-1 B||_F^2  (J space),     B = M^T R^T,  T = R^T R

S is the identity plus a PSD matrix: always positive definite, no threshold, no unit that cannot be scored.  After a pick
C <- C - V V^T (``select.downdate_factor``) and every live unit is scored again; joint scores have no incremental update.

Pure numpy, so that it can be checked without a GPU: ``unit_scores_host`` is the kernel's formulas, ``greedy_joint_host`` the
whole loop; ``select_units`` is the same loop on the resident rows, collective over several ranks.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from .._hostblas import blas_threads
from . import select

CRITERIA = ("gain", "reduction")
EPS = np.finfo(np.float64).eps

UnitSelection = namedtuple("UnitSelection", "keys scores all_keys initial_scores cov dims")
UnitSelection.__doc__ = """Result of ``Solver.select_units``: ``keys`` the picked units in order, ``scores`` each pick's score
(divided by its cost) at the moment it was picked, ``all_keys`` / ``initial_scores`` the one-shot ranking of every unit (this
rank's; an empty unit scores 0), ``cov`` the posterior covariance after the last pick, ``dims`` the order of the Cholesky
factor (min(rows, J)) of every pick."""


def check_criterion(criterion):
    if criterion not in CRITERIA:
        raise ValueError(f"criterion must be one of {CRITERIA}, not {criterion!r}")
    return criterion


def check_criteria(criteria):
    if isinstance(criteria, str):
        criteria = (criteria,)
    return tuple(check_criterion(c) for c in criteria)


def check_cost(unit_cost, ncat):
    """Per-unit costs as a float64 array (None: ones); ValueError unless there is one positive finite cost per unit."""
    if unit_cost is None:
        return np.ones(ncat)
    cost = np.asarray(unit_cost, dtype=np.float64).reshape(-1)
    if cost.shape[0] != ncat:
        raise ValueError(f"{cost.shape[0]} unit costs for {ncat} units")
    if not np.all(np.isfinite(cost)) or not np.all(cost > 0.0):
        raise ValueError("unit_cost must be positive")
    return cost


def factor_cov(cov, rcond=None):
    """M (K x J) with M M^T = cov over the eigenvalues above ``rcond`` (default K eps) times the largest: J is the numerical
    rank, so a pinv covariance with zero columns, or one that a downdate left with a rounding-level negative eigenvalue,
    needs no special case.  A zero covariance gives one zero column."""
    C = np.asarray(cov, dtype=np.float64)
    K = C.shape[0]
    with blas_threads(K):
        lam, U = np.linalg.eigh(0.5 * (C + C.T))
    top = lam[-1] if lam.size else 0.0
    keep = lam > (K * EPS if rcond is None else rcond) * top
    if top <= 0.0 or not keep.any():
        return np.zeros((K, 1))
    return np.ascontiguousarray(U[:, keep][:, ::-1] * np.sqrt(lam[keep][::-1]))


def target_factor(T, rcond=None):
    """R (r x K) with R^T R = T over the eigenvalues above ``rcond`` (default K eps) times the largest; r is the numerical rank
    (0 for T = 0)."""
    T = np.asarray(T, dtype=np.float64)
    K = T.shape[0]
    with blas_threads(K):
        lam, U = np.linalg.eigh(0.5 * (T + T.T))
    top = lam[-1] if lam.size else 0.0
    if not top > 0.0:
        return np.zeros((0, K))
    keep = lam > (K * EPS if rcond is None else rcond) * top
    return np.ascontiguousarray((U[:, keep][:, ::-1] * np.sqrt(lam[keep][::-1])).T)


def gram(rows, scale=None):
    """sum_j s_j t_j t_j^T of target rows on the host."""
    t = np.asarray(rows, dtype=np.float64)
    if scale is None:
        return t.T @ t
    s = np.asarray(scale, dtype=np.float64).reshape(-1)
    if s.shape[0] != t.shape[0]:
        raise ValueError(f"{s.shape[0]} target scales for {t.shape[0]} target rows")
    if np.any(s < 0.0):
        raise ValueError("target scales must not be negative")
    return t.T @ (s[:, None] * t)


def score_one(X, M, tau, B=None, space="auto"):
    """(gain, reduction or None, dim S, n space) of one unit with weighted rows X (n x K): the kernel's formulas."""
    from scipy.linalg import solve_triangular

    X = np.asarray(X, dtype=np.float64).reshape(-1, M.shape[0])
    n, J = X.shape[0], M.shape[1]
    Z = X @ M
    nspace = n <= J if space == "auto" else space == "n"
    G = Z @ Z.T if nspace else Z.T @ Z
    S = G / tau
    S[np.diag_indices_from(S)] += 1.0
    L = np.linalg.cholesky(S)
    g = float(np.log(np.diag(L)).sum())
    red = None
    if B is not None:
        if B.shape[1] == 0:
            red = 0.0
        elif nspace:
            Y = solve_triangular(L, X @ (M @ B), lower=True, check_finite=False)
            red = float((Y * Y).sum() / tau)
        else:
            Y = np.ascontiguousarray(solve_triangular(L, B, lower=True, check_finite=False))   # B's layout: L = I gives 0
            red = float(((B * B).sum(axis=0) - (Y * Y).sum(axis=0)).sum())
    return g, red, L.shape[0], nspace


def unit_layout(cat, ncat):
    """(sorted row ids of the rows with cat >= 0, offsets per unit) of int unit ids per row, rows of a unit in row order."""
    cat = np.asarray(cat)
    order = np.argsort(cat, kind="stable")
    first = np.searchsorted(cat[order], np.arange(ncat + 1))
    return order[first[0]:].astype(np.int32), (first - first[0]).astype(np.int64)


def unit_scores_host(a, cat, ncat, cov, w, noise, T=None, criteria=CRITERIA, alive=None, space="auto", M=None):
    """Scores of every unit in numpy (float64): dict of "gain", "reduction" (arrays over the units, NaN for units that are not
    ``alive``, 0 for empty units; None where not asked for), "dims", "nspace" and "total" = tr(T C).  ``T``: the target Gram
    (needed for the reduction).  ``M``: a factor of ``cov`` to use instead of ``factor_cov(cov)``."""
    criteria = check_criteria(criteria)
    noise = select.check_noise(noise)
    a = np.asarray(a, dtype=np.float64)
    w = np.ones(a.shape[0]) if w is None else np.asarray(w, dtype=np.float64).reshape(-1)
    M = factor_cov(cov) if M is None else M
    B = None
    total = None
    if "reduction" in criteria:
        if T is None:
            raise ValueError("the reduction needs a target")
        B = M.T @ target_factor(T).T
        total = float((B * B).sum())
    rows, off = unit_layout(cat, ncat)
    gain = np.full(ncat, np.nan)
    red = np.full(ncat, np.nan)
    dims = np.zeros(ncat, dtype=np.int64)
    nsp = np.ones(ncat, dtype=bool)
    for u in range(ncat):
        r = rows[off[u]:off[u + 1]]
        if alive is not None and not alive[u]:
            continue
        if r.size == 0:
            gain[u] = red[u] = 0.0
            continue
        g, rd, dims[u], nsp[u] = score_one(w[r, None] * a[r], M, noise, B, space)
        gain[u] = g
        if rd is not None:
            red[u] = rd
    return {"gain": gain if "gain" in criteria else None, "reduction": red if "reduction" in criteria else None, "dims": dims,
            "nspace": nsp, "total": total}


def greedy_joint_host(a, cat, ncat, cov, w, noise, batch_size, criterion="gain", T=None, unit_cost=None):
    """The whole greedy selection in numpy: what ``select_units`` computes with the GPU scoring replaced by
    ``unit_scores_host``.  Returns a dict: "picks" (unit ids), "scores", "gaps" (relative gap to the second-best live score at
    every pick; inf with one live unit), "dims", "cov", "initial" (all scores before the first pick)."""
    criterion = check_criterion(criterion)
    noise = select.check_noise(noise)
    if int(batch_size) < 0:
        raise ValueError("batch_size must not be negative")
    a = np.asarray(a, dtype=np.float64)
    cat = np.asarray(cat)
    w = np.ones(a.shape[0]) if w is None else np.asarray(w, dtype=np.float64).reshape(-1)
    cost = check_cost(unit_cost, ncat)
    C = np.array(cov, dtype=np.float64)
    count = np.bincount(cat[cat >= 0].astype(np.int64), minlength=ncat)
    alive = count > 0
    picks, scores, gaps, dims = [], [], [], []
    initial = None
    for _ in range(int(batch_size) + 1):
        res = unit_scores_host(a, cat, ncat, C, w, noise, T, (criterion,), alive)
        sc = res[criterion] / cost
        if initial is None:
            initial = np.where(count > 0, sc, 0.0)
        if len(picks) == int(batch_size):
            break
        u = select.best_live(sc, alive)
        if u < 0:
            break
        alive[u] = False
        rest = sc[alive]
        gaps.append(float((sc[u] - rest.max()) / abs(sc[u])) if rest.size else np.inf)
        rows = np.flatnonzero(cat == u)
        V = select.downdate_factor(C, w[rows, None] * a[rows], noise)
        C = select.downdate_cov(C, V)
        picks.append(u)
        scores.append(float(sc[u]))
        dims.append(int(res["dims"][u]))
    return {"picks": picks, "scores": scores, "gaps": gaps, "dims": dims, "cov": C, "initial": initial, "alive": alive}


# ---------------------------------------------------------------------------------------------------------------------
# the resident rows
# ---------------------------------------------------------------------------------------------------------------------
def _pool_gram(ctx, m, cat, row_scale):
    """sum s_i a_i a_i^T over the resident rows with cat >= 0 on the GPU: the statistics kernel with weights sqrt(s_i)."""
    s = np.ones(m) if row_scale is None else np.asarray(row_scale, dtype=np.float64).reshape(-1)
    if s.shape[0] != m:
        raise ValueError(f"{s.shape[0]} row scales for {m} rows")
    if np.any(s < 0.0):
        raise ValueError("row_scale must not be negative for the pool target")
    ctx.set_weights(np.where(np.asarray(cat) >= 0, np.sqrt(s), 0.0))
    ctx.resident_train_mask = None               # a fit that follows sends its own weights and mask again
    G, _, _ = ctx.normal_eq()
    return 0.5 * (G + G.T)


def resolve_target(solver, ctx, m, K, cat, row_scale, target):
    """The target Gram T (K x K), summed over the ranks: ``None`` -> this rank's pool rows with ``row_scale`` (on the GPU); a
    row array or ``(rows, scale)`` -> this rank's target rows; ``("gram", T)`` -> T as given (rank 0's on several ranks)."""
    pt = solver.pt
    given = isinstance(target, tuple) and len(target) == 2 and isinstance(target[0], str)
    if given:
        if target[0] != "gram":
            raise ValueError(f"target must be None, rows, (rows, scale) or ('gram', T), not ({target[0]!r}, ...)")
        T = np.array(target[1], dtype=np.float64)
        if T.shape != (K, K):
            raise ValueError(f"the target Gram is {T.shape}, the rows have {K} columns")
        return pt.bcast_object(T, src=0) if pt.multi else T
    if target is None:
        T = _pool_gram(ctx, m, cat, row_scale) if m > 0 else np.zeros((K, K))
    else:
        rows, scale = target if isinstance(target, tuple) else (target, None)
        rows = np.asarray(rows, dtype=np.float64)
        if rows.ndim != 2 or rows.shape[1] != K:
            raise ValueError(f"the target rows have shape {rows.shape}, the pool rows have {K} columns")
        T = gram(rows, scale)
    if pt.multi:
        T = sum(pt.allgather_object(T))
    return T


class _Session:
    """What ``unit_scores`` and ``select_units`` share: the checked inputs, the resident rows and the session on them."""

    def __init__(self, solver, who, a, w, categories, criteria, target, row_scale, unit_cost, noise, cov):
        pt = solver.pt
        self.pt = pt
        self.criteria = criteria
        C = cov if cov is not None else solver.cov
        noise = noise if noise is not None else getattr(solver, "sigmahat", None)
        if pt.multi:
            C, noise = pt.bcast_object((C, noise), src=0)         # rank 0's, where the fit lives
        if C is None:
            raise ValueError(f"{who}: no posterior covariance (fit ANL first, or pass cov=)")
        if noise is None:
            raise ValueError(f"{who}: no noise variance (the sigma^2 of an ANL fit is kept; otherwise pass noise=)")
        self.noise = select.check_noise(noise)
        C = np.array(C, dtype=np.float64)
        if C.ndim != 2 or C.shape[0] != C.shape[1]:
            raise ValueError("cov must be K x K")
        self.C = C
        K = C.shape[0]
        cat, keys = select.category_layout(categories)
        self.cat, self.keys, self.ncat = cat, list(keys), len(keys)
        self.rows_host = pt.shared_arrays["a"].array if a is None else np.asarray(a)
        m = self.rows_host.shape[0]
        if cat.shape[0] != m:
            raise ValueError(f"{cat.shape[0]} categories for {m} rows")
        if m > 0 and self.rows_host.shape[1] != K:
            raise ValueError(f"cov is {K} x {K}, the rows have {self.rows_host.shape[1]} columns")
        if w is None:
            w = pt.shared_arrays["w"].array if a is None else np.ones(m)
        self.w = np.asarray(w, dtype=np.float64).reshape(-1)
        if self.w.shape[0] != m:
            raise ValueError(f"{self.w.shape[0]} weights for {m} rows")
        self.cost = check_cost(unit_cost, self.ncat)
        if pt.multi:
            from . import loco
            try:
                loco.check_units_disjoint(pt.allgather_object(list(keys)))
            except ValueError as e:
                raise ValueError(str(e).replace("loco_errors", who)) from None
        self.sorted_rows, self.offsets = unit_layout(cat, self.ncat)
        self.count = np.diff(self.offsets)
        self.alive = self.count > 0
        self.ctx = solver._uq_rows(a) if m > 0 else None
        self.R = None
        if "reduction" in criteria:
            self.R = target_factor(resolve_target(solver, self.ctx, m, K, cat, row_scale, target))
        self.active = False
        if self.ctx is not None and self.ncat > 0:
            self.ctx.joint_begin(self.sorted_rows, self.offsets, self.w)
            self.active = True

    def score(self):
        """dict of the wanted criteria (per unit, divided by nothing yet; NaN for retired units, 0 for empty ones) + "dims"."""
        out = {"dims": np.zeros(self.ncat, dtype=np.int64)}
        M = factor_cov(self.C)
        B = M.T @ self.R.T if self.R is not None else None
        if self.active:
            if B is not None and B.shape[1] == 0:            # a zero target: no reduction anywhere
                res = self.ctx.joint_score(M, self.noise, None, want_gain="gain" in self.criteria, want_reduction=False)
                res["reduction"] = np.where(self.alive, 0.0, np.nan)
            else:
                res = self.ctx.joint_score(M, self.noise, B, want_gain="gain" in self.criteria,
                                           want_reduction="reduction" in self.criteria)
            out["dims"] = np.where(self.alive, np.nan_to_num(res["info"][:, 0]), 0).astype(np.int64)
        else:
            res = {"gain": np.full(self.ncat, np.nan), "reduction": np.full(self.ncat, np.nan)}
        for c in self.criteria:
            out[c] = np.where(self.count == 0, 0.0, res[c])
        out["total"] = float((B * B).sum()) if B is not None else None
        return out

    def rows_of(self, c):
        rows = self.sorted_rows[self.offsets[c]:self.offsets[c + 1]]
        return self.w[rows, None] * np.asarray(self.rows_host[rows], dtype=np.float64)

    def retire(self, c):
        self.alive[c] = False
        self.ctx.joint_retire(c)

    def end(self):
        if self.active:
            self.ctx.joint_end()
            self.active = False


def unit_scores(solver, a=None, w=None, categories=None, criteria=CRITERIA, target=None, row_scale=None, unit_cost=None,
                noise=None, cov=None):
    """``Solver.unit_scores``: see there."""
    criteria = check_criteria(criteria)
    ses = _Session(solver, "unit_scores", a, w, categories, criteria, target, row_scale, unit_cost, noise, cov)
    try:
        res = ses.score()
    finally:
        ses.end()
    out = {"keys": ses.keys, "count": ses.count.copy(), "dims": res["dims"], "total": res["total"], "gain": None, "reduction": None}
    for c in criteria:
        out[c] = res[c] / ses.cost
    return out


def select_units(solver, batch_size, a=None, w=None, categories=None, criterion="gain", target=None, row_scale=None,
                 unit_cost=None, noise=None, cov=None):
    """``Solver.select_units``: see there."""
    criterion = check_criterion(criterion)
    if int(batch_size) < 0:
        raise ValueError("batch_size must not be negative")
    ses = _Session(solver, "select_units", a, w, categories, (criterion,), target, row_scale, unit_cost, noise, cov)
    pt = solver.pt
    picked, scores, dims = [], [], []
    initial = None
    try:
        for _ in range(int(batch_size) + 1):
            res = ses.score()
            sc = res[criterion] / ses.cost
            if initial is None:
                initial = sc.copy()
            if len(picked) == int(batch_size):
                break
            c = select.best_live(sc, ses.alive)
            s = float(sc[c]) if c >= 0 else 0.0
            if pt.multi:
                pairs = pt.allgather_object((s, c))
                owner, c = select.best_of_ranks(pairs)
                if owner < 0:
                    break
                s = pairs[owner][0]
                msg = None
                if owner == pt._rank:
                    msg = (ses.keys[c], ses.rows_of(c), int(res["dims"][c]))
                    ses.retire(c)
                key, X, d = pt.bcast_object(msg, src=owner)
            else:
                if c < 0:
                    break
                key, X, d = ses.keys[c], ses.rows_of(c), int(res["dims"][c])
                ses.retire(c)
            V = select.downdate_factor(ses.C, X, ses.noise)
            ses.C = select.downdate_cov(ses.C, V)
            picked.append(key)
            scores.append(s)
            dims.append(d)
    finally:
        ses.end()
    return UnitSelection(picked, np.array(scores), ses.keys, initial if initial is not None else np.zeros(0), ses.C, dims)
